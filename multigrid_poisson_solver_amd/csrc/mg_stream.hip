// mg_stream.hip -- the fp64 instantiation of the temporally blocked wave-streaming smoother
// (kernel source and design notes: mg_stream_impl.h).
#define MG_REAL double
#define MG_REAL_NS f64
#include "mg_stream_impl.h"

namespace mg {
namespace k {

int stream_max_steps() { return f64::MAX_S; }
bool stream_supported(int N) { return N >= 3; }
bool stream_fusable(int N) { return N >= 4 && N % 2 == 0; }
bool stream_recompute_supported(int pre, int steps) { return f64::recompute_instantiated(pre, steps); }

void jacobi_stream(hipStream_t s, const SmoothNode<double> &node) { f64::run(s, node); }

}  // namespace k
}  // namespace mg
