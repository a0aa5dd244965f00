// mg_tile_f32.hip -- the fp32 instantiation of the register-tile fused nodes of the small levels (kernel source:
// mg_tile_impl.h): the small levels of the mixed-precision mode's fp32 cycle.  Weights are the fp64 host tables rounded
// to fp32, norms are accumulated in fp64 -- as in mg_stream_f32.hip.
#define MG_REAL float
#define MG_REAL_NS f32
#include "mg_tile_impl.h"

namespace mg {
namespace k {

void jacobi_tile_f32(hipStream_t s, const SmoothNode<float> &node) { f32::tile::run(s, node); }

}  // namespace k
}  // namespace mg
