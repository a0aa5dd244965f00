// mg_tile.hip -- the fp64 instantiation of the register-tile fused nodes of the small levels
// (kernel source and design notes: mg_tile_impl.h).
#define MG_REAL double
#define MG_REAL_NS f64
#include "mg_tile_impl.h"

namespace mg {
namespace k {

// levels the fused driver hands to the tile kernel: MG_TILE_MIN_N <= N <= MG_TILE_MAX_N (defaults 65 and 1024: below, the
// coarse-tail kernel holds the levels in LDS; above, the arrays leave the caches and the streaming kernel's one pass
// over memory wins).  MG_TILE_MAX_N=0 switches the kernel off.
bool tile_wanted(int N)
{
    static const int lo = [] { const char *e = getenv("MG_TILE_MIN_N"); return e ? atoi(e) : 65; }();
    static const int hi = [] { const char *e = getenv("MG_TILE_MAX_N"); return e ? atoi(e) : 1024; }();
    return N >= lo && N <= hi && N >= 16;
}
// a slab of a distributed level is a small launch whatever the level's N: the streaming kernel's launch floor (14-15 us for
// the 256-row slabs of a 2048 level) is what the tile kernel removes
bool tile_wanted_slab(int N)
{
    static const int hi = [] { const char *e = getenv("MG_TILE_SLAB_MAX_N"); return e ? atoi(e) : 2048; }();
    static const int lo = [] { const char *e = getenv("MG_TILE_MIN_N"); return e ? atoi(e) : 65; }();
    return N >= lo && N <= hi && N >= 16;
}
int tile_max_steps() { return f64::tile::MAX_S; }

void jacobi_tile(hipStream_t s, const SmoothNode<double> &node) { f64::tile::run(s, node); }

}  // namespace k
}  // namespace mg
