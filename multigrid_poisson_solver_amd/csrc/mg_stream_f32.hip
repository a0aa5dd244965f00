// mg_stream_f32.hip -- the fp32 instantiation of the temporally blocked wave-streaming smoother
// (kernel source: mg_stream_impl.h): the smoother of the mixed-precision mode (SURVEY.md section
// 8f-2, BASELINE.json config 5: fp32 smoothing, fp64 residual and correction).  Every array and
// every arithmetic operation is fp32 (8 B per lane and row); the transfer weights are the fp64
// host tables rounded to fp32; norms are accumulated in fp64.
#define MG_REAL float
#define MG_REAL_NS f32
#include "mg_stream_impl.h"

namespace mg {
namespace k {

void jacobi_stream_f32(hipStream_t s, const SmoothNode<float> &node) { f32::run(s, node); }

}  // namespace k
}  // namespace mg
