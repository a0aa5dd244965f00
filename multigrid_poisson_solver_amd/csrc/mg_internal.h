// mg_internal.h -- engine-internal declarations shared by the host files and the
// kernel file.  Nothing here is part of the C ABI (include/mg_hip.h).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "mg_hip.h"

namespace mg {

// ---------------------------------------------------------------------------
// errors: the reference printf+exit(1)s (src/MG_solver_GPU.cu:58-62,1286-1289)
// ---------------------------------------------------------------------------
enum ErrorCode {
    MG_OK = 0,
    MG_ERR_HIP = 1,
    MG_ERR_ARG = 2,
    MG_ERR_UNSUPPORTED = 3,
    MG_ERR_NOT_INIT = 4,
    MG_ERR_CYCLE_FILE = 5,
    MG_ERR_COMM = 6,
};

void fail(int code, const char *fmt, ...);
bool hip_ok(hipError_t e, const char *what, const char *file, int line);
#define MG_HIP(expr) ::mg::hip_ok((expr), #expr, __FILE__, __LINE__)

// ---------------------------------------------------------------------------
// device tables for restriction / prolongation, cached per (N, M)
// ---------------------------------------------------------------------------
struct RestrictTable {
    int *lo = nullptr;     // [M] lower-left fine index
    double *w = nullptr;   // [M] weight a (resp. c)
    int *inv = nullptr;    // [N] fine index -> interior coarse index with lo[] == it, else -1
    double *inv_w = nullptr; // [N] w[inv[x]] (0 where inv[x] < 0)
    float *w_f = nullptr, *inv_w_f = nullptr;  // the same weights rounded to fp32 (mixed-precision mode)
    bool fusable = false;  // lo[] strictly increasing by >= 2: one coarse sample per column pair
};
struct ProlongTable {
    int *owner_row = nullptr, *owner_col = nullptr;        // [M]
    double *row_hi = nullptr, *row_lo = nullptr;           // [M] (c3y - f_y), (f_y - c1y)
    double *col_hi = nullptr, *col_lo = nullptr;           // [M] (c2x - f_x), (f_x - c1x)
    float *row_hi_f = nullptr, *row_lo_f = nullptr, *col_hi_f = nullptr, *col_lo_f = nullptr;  // rounded to fp32
    double c_dx = 0.0;
    bool fusable = false;  // every fine index owned, owners advance by <= 1 per fine index
    bool fusable4 = false; // ... and 4 aligned fine columns span at most 3 coarse cells (4 columns per lane, fp32)
    // owner_row[k] == owner_col[k] == min(k*(N-1)/(M-1), N-2) in integer arithmetic for every fine index k (checked entry
    // by entry against the tables built from the reference's ceil() expressions; M <= 4096): a kernel may then form the
    // owner -- an ADDRESS ingredient -- itself instead of waiting for a table load before it can issue its coarse loads
    bool closed_form = false;
};
// a table's weights in the field type: the fp64 array, or its fp32 rounding (the `_f` array)
inline const double *weights_as(double, const double *w, const float *) { return w; }
inline const float *weights_as(float, const double *, const float *w_f) { return w_f; }

// a window of grid rows held in a local array: rows [base, base+rows) of the global grid
// (base may be negative / extend past N: those rows are never touched), of which this rank
// owns [own_lo, own_hi).  1-D row-slab decomposition, BASELINE.json north_star.
struct RowWindow {
    int base = 0, rows = 0, own_lo = 0, own_hi = 0;
    // rows that count towards the error norm; -1: the rows [own_lo, own_hi).  A slab launch may
    // update more rows than its rank owns (redundant halo rows instead of a ghost exchange).
    int norm_lo = -1, norm_hi = -1;
};

// ---------------------------------------------------------------------------
// caching device pool (replaces malloc/free of the level arrays)
// ---------------------------------------------------------------------------
class Pool {
public:
    void *get(size_t bytes);
    void put(void *p);
    void trim();
    size_t bytes_held() const { return held_; }
    // Reuse of a returned block relies on stream order (the next user enqueues behind the last one).  While a cycle plan
    // traces its node program for a batched schedule (mg_cycle.cpp: build_schedule) every visit of a level must keep
    // arrays of its own: with park(true) returned blocks are set aside instead of becoming available, until
    // release_parked() -- called when the schedule is dropped.
    void park(bool on) { park_ = on; }
    void release_parked();
    // MG_POOL_POISON (tests): every block handed out -- fresh or recycled -- is filled with all-ones bytes (a NaN in fp64
    // and in fp32) on the engine's stream first, so that a consumed read of memory nobody wrote shows in the result.
    // Not while that stream is being captured: the fill must not become part of a graph.
    void poison(bool on) { poison_ = on; }
private:
    std::multimap<size_t, void *> free_;   // size -> block
    std::map<void *, size_t> live_;        // block -> size
    std::vector<std::pair<size_t, void *>> parked_;
    bool park_ = false;
    bool poison_ = false;
    size_t held_ = 0;
};
// env MG_POOL_POISON is set (and not "0"): read when a cycle plan or a solver is created
bool pool_poison_wanted();
// all-ones bytes over a device block, enqueued on the engine's stream (skipped while that stream is being captured)
void poison_block(void *p, size_t bytes);

// STREAM_ONLY: the streaming kernel also for a bare single sweep of a large grid (which STREAM hands to the
// one-row-per-block pair kernel): lets the bench report the S = 1 streaming kernel's own rate
enum Smoother { SMOOTHER_STREAM = 0, SMOOTHER_SIMPLE = 1, SMOOTHER_STREAM_ONLY = 2 };

struct NodeOp;   // (below: one fused node launch as the cycle driver's dataflow trace records it)
struct NormSink; // (below: a cycle plan's own store of deferred norm reductions)

struct Context {
    bool ready = false;
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    Pool pool;
    Pool *active_pool = nullptr;           // plan-private arena while a cycle plan executes
    int recompute_min_override = 0;        // > 0 while a batched schedule is traced: the recomputing node pair from this N on
    std::vector<NodeOp> *trace = nullptr;  // != nullptr: fused nodes are recorded, not launched (mg_cycle.cpp: build_schedule)
    bool trace_failed = false;             // ... and one of them was not a single fused launch
    Smoother smoother = SMOOTHER_STREAM;
    int source_mode = 0;                   // mg_set_source: 0 auto (device when it reproduces the host's libm bit for bit), 1 host, 2 device
    int source_identical = -1;             // result of the self-check: -1 not run yet, 0 differs, 1 identical
    // reduction scratch: per-block partial sums + scalar slots
    double *partials = nullptr;
    size_t partials_cap = 0;
    std::vector<void *> retired;          // outgrown scratch, kept alive for captured graphs
    // deferred norm reductions: while a cycle plan runs, the smoothing kernels only leave
    // per-wave partial sums in an arena; ONE kernel per flush finishes all of them
    struct PendingNorm { const double *part; int n; int N; double *out; };
    bool defer_norms = false;
    bool norms_at_window_end = false;      // never flush in mid-window (nodes may still be running on other streams)
    std::vector<PendingNorm> pending_norms;
    double *norm_arena = nullptr;
    size_t norm_arena_cap = 0, norm_arena_used = 0;
    size_t norm_window_total = 0;          // partials requested since the last flush (sizes the arena for the next window)
    NormSink *norm_sink = nullptr;         // != nullptr (while a cycle plan enqueues a window): partials and pending list are the plan's
    double *scalars = nullptr;            // [64] device scalars (errors, norms)
    int *gs_state = nullptr;              // [4]: done flag, iteration count, ...
    double *host_scalars = nullptr;       // pinned [64]
    int *host_ints = nullptr;             // pinned [4]
    std::map<std::pair<int, int>, RestrictTable> rtab;
    std::map<std::pair<int, int>, ProlongTable> ptab;
    int last_error = 0;
    std::string last_error_text;
    bool abort_on_error = true;
    // profiling (mg_profile_begin/end)
    bool profiling = false;
    int profile_min_N = 0;
    int profile_every = 1;                 // mg_profile_sample: time the launches of every k-th cycle window only
    long profile_window = 0;               // windows enqueued since mg_profile_begin
    struct ProfRec { std::string name; int N; double bytes; hipEvent_t e0, e1; };
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;
    // geometry record of the streaming smoother (mg_stream_geometry_log/fetch): MG_STREAM_GEOMETRY_FIELDS ints per launch
    bool geometry_log = false;
    bool geometry_dropped = false;         // the log was full: a record was lost since the last fetch
    std::vector<int> geometry;
};

// live kernel timing: RAII event pair around a launch (no-op unless profiling is on)
struct ProfScope {
    ProfScope(const char *name, int N, double algo_bytes, hipStream_t stream = nullptr);  // nullptr: the engine's stream
    ~ProfScope();
    int slot = -1;
    hipStream_t on = nullptr;
};

Context &ctx();
// one record of the geometry log (the streaming kernel's launcher calls it while ctx().geometry_log is set)
void stream_geometry_record(const int (&rec)[MG_STREAM_GEOMETRY_FIELDS]);
bool require_ready(const char *who);
double *partials(size_t n);   // device scratch for at least n doubles
Pool &scratch_pool();         // where operator-internal scratch comes from
// partial-sum storage + registration of a doSmoothing error reduction (deferred while a plan
// runs, finished immediately otherwise).  flush_norms() finishes everything pending.
double *norm_partials(size_t n);
void norm_finish(hipStream_t s, const double *part, size_t n, int N, double *out);
void flush_norms();
bool stream_is_capturing(hipStream_t s);

// A cycle plan's own store of deferred norm reductions (mg_cycle.cpp).  The plan's launches leave their partial sums in
// blocks from the PLAN'S pool, so nothing another plan, a Solver or an operator call enqueues can overwrite them, and the
// list of pending reductions stays with the plan: a window enqueues no reduction launch at all, mg_cycle_collect finishes
// the last window's -- the only ones anybody reads -- with one launch.  The launches of a plan are the same from window
// to window, so every window walks the blocks the same way and overwrites the partials of the one before it, which
// nobody has read (stream order: a reduction enqueued at collect runs before the next window's kernels).
struct NormSink {
    struct Block { double *p; size_t cap; };
    Pool *pool = nullptr;
    std::vector<Block> blocks;
    size_t block = 0, used = 0;            // where the next partials go
    std::vector<Context::PendingNorm> pending;
    bool unfinished = false;               // a window was enqueued since the pending list was last reduced
    void begin_window();                   // a window's launches follow: back to the first block, an empty list
    double *take(size_t n);
    void flush(hipStream_t s);             // reduce what is pending now and forget it (MAX_NORMS_PER_FLUSH reached in mid-window)
    void finish(hipStream_t s);            // reduce the last window's list if that has not happened yet; the list stays (graph replay)
    void release();                        // the blocks go back to the pool
};

const RestrictTable &restrict_table(int N, int M);
const ProlongTable &prolong_table(int N, int M);
// host-side builders (exact reference expressions)
void build_restriction_table(int N, int M, int *lo, double *w);
void build_prolongation_table(int N, int M, int axis, int *owner, double *w_hi, double *w_lo);
// mg_cubic_table (include/mg_hip.h): long double from the integers, rounded once
void build_cubic_table(int N_src, int N_dst, int *base, double *w);
bool restriction_table_in_bounds(int N, int M, const int *lo);

// getSource (src/MG_solver_CPU.cpp:468-493) for grid rows [row_lo, row_hi) evaluated on the host
// (libm exp) into dev_dst, which points at row row_lo
void fill_source_rows(int N, double L, double min_x, double min_y, int row_lo, int row_hi, double *dev_dst);
// smoothing on a row window with optional fused transfer stages (mg_abi.cpp)
struct SlabFusion {
    const double *coarse = nullptr;
    int Nc = 0;
    double *Fc = nullptr;
    int M = 0;
    RowWindow fine_w, coarse_w, fc_w;
    int pre = 0;          // `1` launch: the pre-smoothed field is recomputed (pre sweeps from zero), U_in is not read
    bool no_out = false;  // `-1` launch: the smoothed field is not stored
    double *out_wide = nullptr;  // fp32 fields: the result goes to this fp64 window (same geometry, exact widening) instead of U_out
};
// T = float: fp32 fields (mixed-precision slabs), and the pointers inside sf are float arrays
template <typename T>
void slab_smooth(int N, double L, const T *U_in, T *U_out, const T *F, int step, double *raw_norm_out, const SlabFusion &sf);

// RCCL transport (mg_comm.cpp)
bool comm_ready();
void comm_set_stream(hipStream_t s);   // stream of the following operations (nullptr: the engine's stream)
int comm_rank();
int comm_size();
void comm_group_begin();
void comm_group_end();
void comm_send(const void *buf, size_t bytes, int peer);   // byte counts: fp64 and fp32 slabs share the transport
void comm_recv(void *buf, size_t bytes, int peer);
void comm_allgather(const double *send, double *recv, size_t count_per_rank);

// small host helper: run fn(begin,end) over [0,n) on the host threads
void parallel_for(size_t n, void (*fn)(size_t, size_t, void *), void *arg, size_t serial_below = 4096);

// A batch of instances of one fused node: the independent visits of one level that a cycle file's dataflow allows to
// run side by side (mg_cycle.cpp: every `-1` node starts from the zero field, so the sub-cycles of a W-cycle below one
// level depend on that level's F alone).  One launch carries all of them: blockIdx.y (coarse tail: blockIdx.x) picks
// the instance, whose arrays come from a table in device memory.  Type-erased: the fp64 and the fp32 kernels share it.
struct NodeBatchItem {
    const void *in, *F, *coarse;   // level-0 input (nullptr: zero / recomputed), source, coarse grid of a fused prolongation
    void *out, *Fc;                // smoothed field, next level's F of a fused restriction
};
struct NodeBatch {
    int n = 0;
    const NodeBatchItem *dev = nullptr;     // [n] in device memory
    double *const *err_outs = nullptr;      // [n] on the host: where each instance's smoothing error goes (device addresses)
};
struct TailBatchItem {
    const void *F_top;
    void *U_top;
    double *err_dev;    // the instance's error slots (node.err_slot counts from here)
    int *gs_state;
};
namespace k {
// One fused smoothing node: level 0 (zero | in | in + P(coarse)), `steps` sweeps, the error norm, optionally the d_sign-ed
// residual of the result stored or restricted.  The launchers (below) take it whole.  A field that a launcher does not
// honour (noted per field) keeps its default; the tile launchers refuse the ones they would ignore.  T is the field type:
// double, or float for the _f32 launchers.
template <typename T>
struct SmoothNode {
    int N = 0;
    T dx2 = 0, inv = 0;               // h^2 and 1/h^2 in the field type
    const T *in = nullptr;            // level-0 input (nullptr: all zero; not read when pre > 0)
    const T *F = nullptr;
    T *out = nullptr;                 // the smoothed field
    int steps = 0;                    // sweeps in this launch: 1..stream_max_steps() / 1..tile_max_steps()
    double *err = nullptr;            // device slot of the smoothing error (fp64); with fine_w its raw sum over the counted rows
    T *D = nullptr;                   // the d_sign-ed residual of the result, stored (streaming launchers only)
    int d_sign = -1;                  // sign of the residual in D and of the one restricted into Fc
    const T *coarse = nullptr;        // level 0 is in + doProlongation(coarse), Nc x Nc, with the tables pt
    int Nc = 0;
    const ProlongTable *pt = nullptr;
    T *Fc = nullptr;                  // the residual restricted into Fc, M x M, with the tables rt
    int M = 0;
    const RestrictTable *rt = nullptr;
    // row windows of the fine arrays, of coarse and of Fc for the 1-D row-slab decomposition (nullptr: the whole grid is local)
    const RowWindow *fine_w = nullptr, *coarse_w = nullptr, *fc_w = nullptr;
    int pre = 0;                      // fused `1` node: in is recomputed as pre sweeps from zero on F (streaming only)
    bool no_out = false;              // fused `-1` node: out is not stored (its `1` node recomputes it)
    double *out_wide = nullptr;       // the result goes to this fp64 array (exact widening) instead of out (jacobi_stream_f32)
    // the same node on batch->n instances in one launch (jacobi_stream, jacobi_tile): in/F/out/coarse/Fc above then only tell
    // the node's shape -- which of them a node of this kind has -- and err is ignored
    const NodeBatch *batch = nullptr;
    // != 0.25: the weighted sweep U + (cw*t) of the residual-tolerance solver (cw = 0.25*omega; jacobi_stream, no recomputing
    // pair); 0.25 is the reference's sweep
    double cw = 0.25;
    // shifted: the screened operator of the residual-tolerance solver (mg_solve_opts.shift != 0): the centre coefficient of
    // the bracket is dc = 4 + shift*dx2 (product rounded, then subtracted) in the sweeps and in the residual stage, and cw
    // is omega/dc; always a weighted instantiation
    double dc = 4.0;
    bool shifted = false;
};
// centre coefficient d = 4 + shift*dx2 and q = 1/d of one level of the screened operator (mg_solve.cpp: LevelConsts) for
// the solver's operator-by-operator kernels; on = false (shift == 0): the unshifted kernels, d and q are not looked at
struct Shifted {
    bool on = false;
    double d = 4.0, q = 0.25;
};
}  // namespace k

// One fused node launch as the cycle driver's dataflow trace records it (mg_cycle.cpp: build_schedule): while
// Context::trace is set, the fused-node entry points describe their launch here instead of enqueueing it.
struct NodeOp {
    int kind = 0;                 // 0: streaming kernel, 1: register-tile kernel, 2: coarse tail (tail = index of its TailArgs)
    double L = 1.0;
    k::SmoothNode<double> node;   // the launch (a coarse tail: N, F, out)
    int tail = -1;
    char name[48] = {0};
    double bytes = 0.0;
};

// ---------------------------------------------------------------------------
// kernel launchers (mg_kernels.hip).  All enqueue on s and return immediately.
// ---------------------------------------------------------------------------
namespace k {
// one Jacobi sweep in correction form, in -> out (in == nullptr: all zero)
void jacobi_simple(hipStream_t s, int N, double dx2, const double *in, const double *F, double *out);
// D = sign * (inv*(star - 4U) - F), rim sign*0
// (sh.on: the bracket's centre term is sh.d*U, the residual-tolerance solver's screened operator)
void residual(hipStream_t s, int N, double inv, const double *U, const double *F, double *D, int sign, const Shifted &sh = {});
// doSmoothing's error: *out = (S+S)/N/N, S = sum over (row+col) even interior of |inv*star-F|
void smoothing_error(hipStream_t s, int N, double inv, const double *U, const double *F, double *out);
// second stage of doSmoothing's error: *out = (sum+sum)/N/N over n per-block partials
void finish_smoothing_error(hipStream_t s, const double *part, size_t n, int N, double *out);
constexpr int MAX_NORMS_PER_FLUSH = 160;   // (the descriptors travel as kernel arguments: 24 B each, 4 KB at most)
struct NormBatch {
    const double *part[MAX_NORMS_PER_FLUSH];
    double *out[MAX_NORMS_PER_FLUSH];
    int n[MAX_NORMS_PER_FLUSH];
    int N[MAX_NORMS_PER_FLUSH];
};
void finish_smoothing_errors(hipStream_t s, const NormBatch &b, int count);
// temporally blocked streaming smoother (mg_stream.hip): steps <= stream_max_steps()
int  stream_max_steps();
bool stream_supported(int N);
bool stream_fusable(int N);   // the fused prolongation / restriction stages exist for this N
// the recomputing fused `1` node (pre sweeps from zero redone in flight, then `steps` more) is instantiated for this pair
// in THIS build (it depends on the prefetch depth the library was compiled with, MG_PF)
bool stream_recompute_supported(int pre, int steps);
void jacobi_stream(hipStream_t s, const SmoothNode<double> &node);
// register-tile fused nodes of the small levels (mg_tile.hip / mg_tile_f32.hip): the node in one launch, without a stored
// residual and without the recomputing or the weighted form
bool tile_wanted(int N);      // MG_TILE_MIN_N <= N <= MG_TILE_MAX_N
bool tile_wanted_slab(int N); // the same for a launch on a row window (a slab of a distributed level): up to MG_TILE_SLAB_MAX_N
int  tile_max_steps();
void jacobi_tile(hipStream_t s, const SmoothNode<double> &node);
void jacobi_tile_f32(hipStream_t s, const SmoothNode<float> &node);
void restrict_gather(hipStream_t s, int N, const double *Uf, int M, double *Uc, const RestrictTable &t, int sign);
// Uf_out = (Uf_in ? Uf_in : 0) + P(Uc); when Uf_in == nullptr unowned fine points are left untouched
void prolong(hipStream_t s, int N, const double *Uc, int M, const double *Uf_in, double *Uf_out, const ProlongTable &t);
void restrict_gather_f32(hipStream_t s, int N, const float *Uf, int M, float *Uc, const RestrictTable &t, int sign);
void prolong_add_f32(hipStream_t s, int N, const float *Uc, int M, const float *Uf_in, float *Uf_out, const ProlongTable &t);
void convert_to_f32(hipStream_t s, float *dst, const double *src, size_t n);
void convert_to_f64(hipStream_t s, double *dst, const float *src, size_t n);
void refine_residual(hipStream_t s, int N, double inv, const double *U, const double *F, float *src, double *err_out);
void add_widened(hipStream_t s, double *U, const float *e, size_t n);
void refine_residual_rows(hipStream_t s, int N, double inv, const double *U, const double *F, float *src, const RowWindow &w,
                          double *out_raw);
void add(hipStream_t s, size_t n, double *a, const double *b);
void negate(hipStream_t s, size_t n, double *a);
// F points at row row_lo; rows [row_lo, row_hi)
void source_device(hipStream_t s, int N, double L, double *F, double min_x, double min_y, int row_lo, int row_hi);
void analytic(hipStream_t s, int N, double L, double *U, double min_x, double min_y);
void analytic_error(hipStream_t s, int N, double L, const double *U, double min_x, double min_y, double *out);
// raw sum |analytic - U| over the owned rows of a row window (combined across slabs by the caller)
void analytic_error_rows(hipStream_t s, int N, double L, const double *U, const RowWindow &w, double min_x,
                         double min_y, double *out_raw);
void fill_uniform(hipStream_t s, double *dst, size_t n, uint64_t seed);
void checksum(hipStream_t s, const double *src, size_t n, uint64_t *out_dev /*[2]*/);
// fp32 instantiation of the streaming smoother (mg_stream_f32.hip)
void jacobi_stream_f32(hipStream_t s, const SmoothNode<float> &node);
// coarse tail of a cycle in one launch (mg_tail.hip): the node slice that stays on levels N <= 64
constexpr int TAIL_MAX_LEVELS = 6;
constexpr int TAIL_MAX_NODES = 48;
constexpr int TAIL_MAX_N = 64;
struct TailNode {
    int type;      // -1, 0, 1
    int steps;     // smoothing steps (-1 / 1)
    int err_slot;  // index into err_dev, or -1
    int pad;
    double tol;    // exact-solver target (0)
};
template <typename T>
struct TailArgsT {
    int n_levels, n_nodes;
    int N[TAIL_MAX_LEVELS];
    T dx2[TAIL_MAX_LEVELS], inv[TAIL_MAX_LEVELS];
    double gs_h2[TAIL_MAX_LEVELS], gs_inv[TAIL_MAX_LEVELS];  // fp64 spacings: the exact solver is fp64 in every mode
    const int *r_lo[TAIL_MAX_LEVELS];      // restriction level l -> l+1
    const T *r_w[TAIL_MAX_LEVELS];
    const int *p_orow[TAIL_MAX_LEVELS], *p_ocol[TAIL_MAX_LEVELS];  // prolongation level l+1 -> l
    const T *p_rhi[TAIL_MAX_LEVELS], *p_rlo[TAIL_MAX_LEVELS], *p_chi[TAIL_MAX_LEVELS], *p_clo[TAIL_MAX_LEVELS];
    T c_dx[TAIL_MAX_LEVELS];
    int tab_real0, tab_int0;  // where the staged tables start in LDS (set by the launcher)
    long long *trace;         // diagnostics (MG_TAIL_TRACE): 100 MHz timestamps at start, after staging, after each node
    const T *F_top;
    T *U_top;
    double *err_dev;   // norms are fp64 whatever the field type
    int *gs_state;
    const TailBatchItem *batch;   // != nullptr: blockIdx.x picks the instance's F_top / U_top / err_dev / gs_state
    TailNode nodes[TAIL_MAX_NODES];
};
typedef TailArgsT<double> TailArgs;
typedef TailArgsT<float> TailArgsF;
void tail_launch_f32(hipStream_t s, const TailArgsF &a);
bool tail_fits(const TailArgs &a);
void tail_launch(hipStream_t s, const TailArgs &a, int n_batch = 1, const TailBatchItem *batch_dev = nullptr);
// red-black Gauss-Seidel to tolerance, fully on device; iterations -> state[1]
void gauss_seidel(hipStream_t s, int N, double h2, double inv, double *U, const double *F, double tol,
                  int *state);
void gauss_seidel_blocks_launch(hipStream_t s, int N, double h2, double inv, double *U, const double *F, double tol, int *state);
int  gs_single_workgroup_max_n();
// residual-tolerance solver (mg_solve_kernels.hip, driven by mg_solve.cpp)
// one weighted Jacobi sweep U = U_old + cw*(star - 4 U_old - dx^2 F), cw = 0.25*omega, rim kept (in == nullptr: all zero)
// sh.on: the bracket's centre term is sh.d*U_old (rounded, then subtracted) and cw = omega*sh.q
void wjacobi(hipStream_t s, int N, double dx2, double cw, const double *in, const double *F, double *out, const Shifted &sh = {});
// *out = sqrt(sum over interior points of d^2), d = inv*(star - 4U) - F (U == nullptr: d = F); part holds at least
// resnorm_partials(N) doubles; the partials are summed in a fixed order (bit-reproducible)
size_t resnorm_partials(int N);
void resnorm(hipStream_t s, int N, double inv, const double *U, const double *F, double *part, double *out, const Shifted &sh = {});
// red-black Gauss-Seidel from zero to err <= max(atol, rtol*err0) (err0: the metric at U = 0), 1 ... max_iters iterations,
// one workgroup; state[1] = iterations, state[2] = 1 when the cap ended it above the target; err_out[0..1] = err0, err
constexpr int GS_RELATIVE_MAX_N = 64;
bool gs_relative_fits(int N);
// sh.on: update sh.q*(... - h^2 F), error metric with the centre term sh.d*U
void gauss_seidel_relative(hipStream_t s, int N, double h2, double inv, double *U, const double *F, double atol, double rtol,
                           int max_iters, int *state, double *err_out, const Shifted &sh = {});
// the same kernels on n instances of one size in ONE launch each (batched solver, mg_solve_batch.cpp): items[i] (device
// memory) holds instance i's arrays, each instance runs exactly the code and the partition of its single-instance form.
// resnorm_batch: in = U (has_u), F; out[i] = its norm, its partials at part + i*resnorm_partials(N)
void resnorm_batch(hipStream_t s, int n, int N, double inv, bool has_u, const NodeBatchItem *items, double *part, double *out,
                   const Shifted &sh = {});
// out = U, F; instance i's state at state + 4i (no err_out)
void gauss_seidel_relative_batch(hipStream_t s, int n, int N, double h2, double inv, const NodeBatchItem *items, double atol,
                                 double rtol, int max_iters, int *state, const Shifted &sh = {});
// residual (in = U, F, out = D), restriction N -> M (in -> out), out = in + prolongation of coarse (N -> M), copy in -> out
void residual_batch(hipStream_t s, int n, int N, double inv, const NodeBatchItem *items, int sign, const Shifted &sh = {});
void restrict_batch(hipStream_t s, int n, int N, int M, const NodeBatchItem *items, const RestrictTable &t, int sign);
void prolong_add_batch(hipStream_t s, int n, int N, int M, const NodeBatchItem *items, const ProlongTable &t);
void copy_batch(hipStream_t s, int n, size_t count, const NodeBatchItem *items);
// full-multigrid start of the residual-tolerance solver (mg_fmg_kernels.hip, driven by mg_solve.cpp: fmg_start).
// CubicTable: mg_cubic_table(N_src -> N_dst) in device memory, base[N_dst] and w[N_dst][4]; one table serves rows and columns.
struct CubicTable {
    int N_src = 0, N_dst = 0;
    int *base = nullptr;
    double *w = nullptr;
};
// the block tiling of prolong_cubic holds every source window of this table (checked on the host when the table is made)
bool cubic_table_fits(int N_src, int N_dst, const int *base_host);
// interior of Uf (N_dst x N_dst) = bicubic interpolation of Uc (N_src x N_src, rim included as data); the rim of Uf is not written
void prolong_cubic(hipStream_t s, const CubicTable &t, const double *Uc, double *Uf);
// the rim of an N x N array as four edges g[0..4N): row 0, row N-1, column 0, column N-1
void rim_extract(hipStream_t s, int N, const double *U, double *g);
// the edges of the coarse rim sampled from the fine edges with the 1-D table t (fine -> coarse), corners included
void rim_sample(hipStream_t s, const CubicTable &t, const double *g_f, double *g_c);
// rim of U = g; zero_interior: the interior is set to +0 (rim_only), otherwise it is not written
void rim_fill(hipStream_t s, int N, const double *g, double *U, bool zero_interior);
// *acc = 1 when gs_state[2] (the coarse solve ended at its cap) is set
void flag_or(hipStream_t s, const int *gs_state, int *acc);
// right-hand side of a theta-scheme time step of the heat equation (mg_heat_kernels.hip, driven by mg_heat.cpp; the
// expression and its order: include/mg_heat.h).  lap = false (theta == 1): the Laplacian term is left out, no neighbour is read
struct HeatConsts {
    double sigma = 0.0, beta = 0.0, gamma = 0.0, inv = 0.0;
    bool lap = false;
};
// F = rhs(U, Q) (Q == nullptr: no source); the rim of F is +0, nothing else is written
void heat_rhs(hipStream_t s, int N, const HeatConsts &c, const double *U, const double *Q, double *F);
// the same on n instances in one launch: in = U, coarse = Q (may be null per instance), out = F
void heat_rhs_batch(hipStream_t s, int n, int N, const HeatConsts &c, const NodeBatchItem *items);
// the residual-tolerance solver with a variable coefficient (mg_varcoef_kernels.hip, driven by mg_solve.cpp; the expressions
// and their order: include/mg_varcoef.h).  A: the level's nodal coefficient, sd = shift*dx2 of the level.
// one sweep U = U_old + omega*q*(b(U_old) - dx2*F), q = 1/d formed per point (in == nullptr: from the zero field)
void wjacobi_vc(hipStream_t s, int N, double dx2, double sd, double omega, const double *A, const double *in, const double *F,
                double *out);
// D = sign * (inv*b(U) - F), rim sign*0
void residual_vc(hipStream_t s, int N, double inv, double sd, const double *A, const double *U, const double *F, double *D, int sign);
// out = inv*b(U), rim +0 (A == nullptr: a = 1)
void apply_vc(hipStream_t s, int N, double inv, double sd, const double *A, const double *U, double *out);
// *out = sqrt(sum over interior points of (inv*b(U) - F)^2) in the partition and order of resnorm (part: resnorm_partials(N))
void resnorm_vc(hipStream_t s, int N, double inv, double sd, const double *A, const double *U, const double *F, double *part,
                double *out);
// gauss_seidel_relative with the variable operator (N < GS_RELATIVE_MAX_N; the same LDS request)
void gauss_seidel_relative_vc(hipStream_t s, int N, double h2, double inv, double sd, const double *A, double *U, const double *F,
                              double atol, double rtol, int max_iters, int *state, double *err_out);
// Ac (M x M) = the nodal coefficient Af (N x N) sampled with t = restrict_table(N, M), rim included, clamped to its samples
void coef_coarsen(hipStream_t s, int N, const double *Af, int M, double *Ac, const RestrictTable &t);
// *flag = 1 when a value of A[0..n) is not finite or not > 0 (the caller zeroes the flag)
void coef_check(hipStream_t s, const double *A, size_t n, int *flag);
// batched forms of the above (mg_varcoef_batch_kernels.hip, driven by mg_solve_batch.cpp): one launch over n instances, each
// running the code and the block partition of its single launch (the bodies are shared: mg_varcoef_impl.h).  items[i]: the
// arrays of instance i, the level's coefficient in the slot `coarse`.
// sweep: in = U (zero_in: not read), F, coarse = a, out
void wjacobi_vc_batch(hipStream_t s, int n, int N, double dx2, double sd, double omega, bool zero_in, const NodeBatchItem *items);
// residual: in = U, F, coarse = a, out = D
void residual_vc_batch(hipStream_t s, int n, int N, double inv, double sd, const NodeBatchItem *items, int sign);
// norm: in = U, F, coarse = a; out[i] = its norm, its partials at part + i*resnorm_partials(N)
void resnorm_vc_batch(hipStream_t s, int n, int N, double inv, double sd, const NodeBatchItem *items, double *part, double *out);
// coarse solve: out = U, F, coarse = a; instance i's state at state + 4i (no err_out)
void gauss_seidel_relative_vc_batch(hipStream_t s, int n, int N, double h2, double inv, double sd, const NodeBatchItem *items,
                                    double atol, double rtol, int max_iters, int *state);
// coarsening N -> M: in = a_f, out = a_c; check of `count` values: in = a, flags[i] = 1 for a bad instance (zeroed by the caller)
void coef_coarsen_batch(hipStream_t s, int n, int N, int M, const NodeBatchItem *items, const RestrictTable &t);
void coef_check_batch(hipStream_t s, int n, size_t count, const NodeBatchItem *items, int *flags);
// right-hand side of a theta-scheme time step with a variable coefficient (mg_heat_vc_kernels.hip, driven by mg_heat.cpp; the
// expression and its order: include/mg_heat_vc.h).  c.lap must be set: theta == 1 reads no coefficient and goes to heat_rhs.
// F = rhs(A, U, Q) (Q == nullptr: no source); the rim of F is +0, nothing else is written
void heat_rhs_vc(hipStream_t s, int N, const HeatConsts &c, const double *A, const double *U, const double *Q, double *F);
// boundary kinds per side (mg_bc_kernels.hip, driven by mg_solve.cpp and mg_heat.cpp; the expressions and their order:
// include/mg_bc.h).  kind: host int[4], S, N, W, E, each 0 (Dirichlet) or 1 (Neumann); A == nullptr: a = 1.  The `_vc`
// launchers above with the unknowns in the interior's place and mirrored neighbours beyond a Neumann side.
void wjacobi_bc(hipStream_t s, int N, double dx2, double sd, double omega, const int *kind, const double *A, const double *in,
                const double *F, double *out);
void residual_bc(hipStream_t s, int N, double inv, double sd, const int *kind, const double *A, const double *U, const double *F,
                 double *D, int sign);
void apply_bc(hipStream_t s, int N, double inv, double sd, const int *kind, const double *A, const double *U, double *out);
// *out = the L2 norm of the residual over the unknowns (U == nullptr: of F), partition and order of resnorm
void resnorm_bc(hipStream_t s, int N, double inv, double sd, const int *kind, const double *A, const double *U, const double *F,
                double *part, double *out);
void gauss_seidel_relative_bc(hipStream_t s, int N, double h2, double inv, double sd, const int *kind, const double *A, double *U,
                              const double *F, double atol, double rtol, int max_iters, int *state, double *err_out);
// the singular problem (include/mg_singular.h; kind: four Neumann sides, sd = 0): the same solve on F minus its weighted mean
// m_c, which goes to *mean_out (device memory, may be nullptr); F itself is not written
void gauss_seidel_relative_bc_mean(hipStream_t s, int N, double h2, double inv, const int *kind, const double *A, double *U,
                                   const double *F, double atol, double rtol, int max_iters, int *state, double *err_out,
                                   double *mean_out);
// the weighted mean and the shift of include/mg_singular.h (mg_singular_kernels.hip).  weighted_mean: out[0] = mean_w(X),
// out[1] = mean_w(X) - target, summed over part (resnorm_partials(N) doubles) in the header's order; shift_by: Xout = Xin - *c
// (Xout may be Xin)
void weighted_mean(hipStream_t s, int N, const double *X, double target, double *part, double *out);
void shift_by(hipStream_t s, int N, const double *Xin, const double *c, double *Xout);
// Fc (M x M) = the restriction of D (N x N) at the coarse unknowns, +0 at coarse data points; t = restrict_table(N, M)
void restrict_bc(hipStream_t s, int N, const int *kind, const double *D, int M, double *Fc, const RestrictTable &t);
// Uout = Uin + P(Uc) at the fine unknowns, Uin at fine data points; lo, w: mg_boundary_prolongation_table(M, N) in device memory
void prolong_add_bc(hipStream_t s, int M, const int *kind, const double *Uc, int N, const double *Uin, double *Uout, const int *lo,
                    const double *w);
// Fout = F - (t*a)*g at the rim unknowns of Neumann sides (G: 4 x N, rows S, N, W, E), a copy elsewhere
void neumann_source(hipStream_t s, int N, double t, const int *kind, const double *A, const double *F, const double *G, double *Fout);
// the heat right-hand side at the unknowns, +0 at data points (c.lap == false: no neighbour and no coefficient is read)
void heat_rhs_bc(hipStream_t s, int N, const HeatConsts &c, const int *kind, const double *A, const double *U, const double *Q,
                 double *F);
// the residual-tolerance solver with a variable reaction term (mg_reaction_kernels.hip, driven by mg_solve.cpp; the expressions
// and their order: include/mg_reaction.h).  The `_vc` launchers above with the centre's shift term formed per point, sd + S*dx2:
// S is the level's nodal reaction term, A its coefficient or nullptr (a = 1 through the same expressions, nothing streamed
// for it); every launcher takes dx2 beside inv for that product.
void wjacobi_rx(hipStream_t s, int N, double dx2, double sd, double omega, const double *A, const double *S, const double *in,
                const double *F, double *out);
void residual_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U,
                 const double *F, double *D, int sign);
void apply_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U, double *out);
void resnorm_rx(hipStream_t s, int N, double dx2, double inv, double sd, const double *A, const double *S, const double *U,
                const double *F, double *part, double *out);
void gauss_seidel_relative_rx(hipStream_t s, int N, double h2, double inv, double sd, const double *A, const double *S, double *U,
                              const double *F, double atol, double rtol, int max_iters, int *state, double *err_out);
// *flag = 1 when a value of S[0..n) is not finite or not >= 0 (the caller zeroes the flag)
void reaction_check(hipStream_t s, const double *S, size_t n, int *flag);
// batched forms of the above (mg_reaction_batch_kernels.hip, driven by mg_solve_batch.cpp; include/mg_rx_batch.h): one launch
// over n instances, each running the code and the block partition of its single launch (the bodies are shared:
// mg_reaction_impl.h).  items[i]: the arrays of instance i as the `_vc_batch` launchers take them, the level's reaction term in
// the slot `Fc`; has_a: the slot `coarse` of EVERY instance holds its coefficient (false: it is not read, a = 1).
void wjacobi_rx_batch(hipStream_t s, int n, int N, double dx2, double sd, double omega, bool zero_in, bool has_a, const NodeBatchItem *items);
void residual_rx_batch(hipStream_t s, int n, int N, double dx2, double inv, double sd, bool has_a, const NodeBatchItem *items, int sign);
// A*z: in = z, coarse = a, Fc = s, out
void apply_rx_batch(hipStream_t s, int n, int N, double dx2, double inv, double sd, bool has_a, const NodeBatchItem *items);
void resnorm_rx_batch(hipStream_t s, int n, int N, double dx2, double inv, double sd, bool has_a, const NodeBatchItem *items, double *part,
                      double *out);
void gauss_seidel_relative_rx_batch(hipStream_t s, int n, int N, double h2, double inv, double sd, bool has_a, const NodeBatchItem *items,
                                    double atol, double rtol, int max_iters, int *state);
// check of `count` values: in = s, flags[i] = 1 for an instance with a value that is not finite or not >= 0 (zeroed by the caller)
void reaction_check_batch(hipStream_t s, int n, size_t count, const NodeBatchItem *items, int *flags);
// the pass of the semilinear solve (mg_newton_kernels.hip, driven by mg_solve.cpp; the expressions and their order:
// include/mg_newton.h): V = U + t*dlt (dlt == nullptr: no step, V not written), S = kappa*W*g'(V) on all N^2 points,
// D = (F + kappa*W*g(V)) - inv*b(V) inside and +0 on the rim, *out = sqrt(sum of D^2) in the partition and order of resnorm
// (part: resnorm_partials(N)).  kind: MG_NEWTON_*; A, W: nullptr for a = 1, w = 1, nothing streamed for either.
void newton_residual(hipStream_t s, int N, double inv, double sd, int kind, double kappa, const double *A, const double *W,
                     const double *U, const double *dlt, double t, const double *F, double *V, double *D, double *S, double *part,
                     double *out);
// the batched form of the pass (mg_newton_batch_kernels.hip, driven by mg_solve_batch.cpp; include/mg_newton_batch.h): one launch
// over n instances, each running the code, the block partition and the summation order of its single launch (the bodies are
// shared: mg_newton_impl.h).  items[z]: the arrays and the kappa of the instance in slot z; has_a / has_w / has_step: EVERY
// instance's A / W / (dlt, V) is there (false: the slot is not read).  Partials at part + z*resnorm_partials(N), norms to out[z].
struct NewtonBatchItem {
    const double *A, *W, *U, *dlt, *F;
    double *V, *D, *S;
    double kappa;
};
void newton_residual_batch(hipStream_t s, int n, int N, double inv, double sd, int kind, bool has_a, bool has_w, bool has_step, double t,
                           const NewtonBatchItem *items, double *part, double *out);
// Krylov acceleration of the residual-tolerance solver (mg_krylov_kernels.hip, driven by mg_solve.cpp; the method and the
// order of every operation: include/mg_krylov.h).  All sums run over the interior; no rim is read into a result or written.
constexpr int KRYLOV_MAX_K = MG_KRYLOV_MAX_M - 1;   // stored directions an iteration orthogonalises against
struct KrylovVecs {
    const double *q[KRYLOV_MAX_K];
    const double *z[KRYLOV_MAX_K];
};
// blocks of one launch over an N x N grid: every sum needs this many partials
size_t krylov_blocks(int N);
// d_out[j] = <q, v.q[j]> and, where w is given, b[j] = d_out[j]*w[j], j < k (1 <= k <= KRYLOV_MAX_K; part: k*krylov_blocks(N))
void krylov_dots(hipStream_t s, int N, int k, const double *q, const KrylovVecs &v, double *part, const double *w, double *b,
                 double *d_out);
// q -= b[j]*v.q[j], z -= b[j]*v.z[j] for j = 0 .. k-1 in order (b: device, k doubles); the partials of <q, q> and <r, q> into
// part (2*krylov_blocks(N))
void krylov_orth(hipStream_t s, int N, int k, double *q, double *z, const double *r, const KrylovVecs &v, const double *b,
                 double *part);
// gh[0..1] = g, h.  alpha != nullptr (a solve): *w_k = 1/g, *alpha = h/g or 0 with *brk = 1.0 on a breakdown (else 0.0), and
// where rec is given the head of the log record of m + 7 doubles
void krylov_orth_finish(hipStream_t s, int N, const double *part, int k, int m, double *gh, double *w_k, double *alpha, double *brk,
                        double *rec);
// U += alpha*z, r -= alpha*q (*alpha == 0: neither is written); the partials of <r, r> into part (krylov_blocks(N))
void krylov_update(hipStream_t s, int N, const double *alpha, double *U, const double *z, double *r, const double *q, double *part);
// rr != nullptr: *rr = <r, r>.  rho_out != nullptr (a solve): *rho_out = sqrt of it, rec_tail[0..2] = rho_rec, 0, rho_rec
void krylov_update_finish(hipStream_t s, int N, const double *part, double *rr, double *rho_out, double *rec_tail);
// a restart's mark in the log record: rec_tail[1] = 1, rec_tail[2] = *rho
void krylov_log_restart(hipStream_t s, double *rec_tail, const double *rho);
// batched forms of the above (mg_krylov_batch_kernels.hip, driven by mg_solve_batch.cpp; include/mg_krylov_batch.h): one
// launch over n instances, each running the code, the block partition and the summation order of its single launch (the
// bodies are shared: mg_krylov_impl.h).  items[slot]: the arrays of the instance in that active slot; v: the slots of the
// stored directions, each holding every instance at the instance pitch.
struct KrylovBatchItem {
    double *U, *r;       // the caller's U, the instance's residual
    double *zk, *qk;     // this iteration's z_k, q_k
    double *scal;        // its scalars, KRYLOV_SCAL_COUNT doubles
    double *part;        // its partials, KRYLOV_MAX_K*krylov_blocks(N)
    double *rec;         // its log record of this iteration, m + 7 doubles
    size_t off;          // its offset (doubles) in every slot of the stored directions: z_j = v.z[j] + off
    int k, pad;          // its stored directions so far
};
constexpr int KRYLOV_SCAL_B = 0, KRYLOV_SCAL_W = MG_KRYLOV_MAX_M, KRYLOV_SCAL_ALPHA = 2 * MG_KRYLOV_MAX_M,
              KRYLOV_SCAL_BRK = KRYLOV_SCAL_ALPHA + 1, KRYLOV_SCAL_COUNT = KRYLOV_SCAL_ALPHA + 2;
// z_k = +0, all N*N doubles
void krylov_zero_batch(hipStream_t s, int n, int N, const KrylovBatchItem *items);
// d_j = <q_k, q_j> into the record and b_j = d_j*w_j, j < the instance's k; kmax: the largest k of the n instances
// (1 .. KRYLOV_MAX_K; instances at k = 0 are left alone).  Two launches.
void krylov_dots_batch(hipStream_t s, int n, int N, int kmax, const KrylovBatchItem *items, const KrylovVecs &v);
// the orthogonalisation against the instance's k directions, g, h, w_k, alpha, the breakdown flag and the head of the
// record (kmax: 0 .. KRYLOV_MAX_K).  Two launches.
void krylov_orth_batch(hipStream_t s, int n, int N, int kmax, int m, const KrylovBatchItem *items, const KrylovVecs &v);
// U += alpha*z_k, r -= alpha*q_k, rho_rec and the tail of the record; rb[slot] = rho_rec, rb[stride + slot] = the breakdown
// flag.  Two launches.
void krylov_update_batch(hipStream_t s, int n, int N, int m, const KrylovBatchItem *items, double *rb, int stride);
// a restart's mark in the records of n restarting instances: restarted = 1, rho = norms[slot]
void krylov_log_restart_batch(hipStream_t s, int n, int m, const KrylovBatchItem *items, const double *norms);
// A*z for n instances: in = z, coarse = a (nullptr for that instance: a = 1), out (mg_varcoef_batch_kernels.hip: apply_vc's body)
void apply_vc_batch(hipStream_t s, int n, int N, double inv, double sd, const NodeBatchItem *items);
// adjoint sensitivities (mg_adjoint_kernels.hip, driven by mg_adjoint.cpp; the expressions and their order:
// include/mg_adjoint.h).  gA = the gradient in the nodal coefficient at every grid point, h = 0.5*inv; the rim of lam is
// substituted by +0.0, never used from memory
void coef_grad(hipStream_t s, int N, double h, const double *lam, const double *U, double *gA);
// gU = the gradient in the rim data: +0 on the interior, Ubar at the corners, Ubar - inv*(f*lam[p]) on the rest of the rim
// (A == nullptr: a = 1; Ubar == nullptr: 0.0)
void rim_grad(hipStream_t s, int N, double inv, const double *A, const double *lam, const double *Ubar, double *gU);
// the same on n instances in one launch each: in = lam, F = U, out = gA / in = lam, F = Ubar, coarse = a (both may be null
// per instance), out = gU
void coef_grad_batch(hipStream_t s, int n, int N, double h, const NodeBatchItem *items);
void rim_grad_batch(hipStream_t s, int n, int N, double inv, const NodeBatchItem *items);
// lowest eigenmodes, LOBPCG (mg_eigs_kernels.hip, driven by mg_eigs.cpp; the method and the order of every operation:
// include/mg_eigs.h).  All sums run over the interior; no rim is read into a result or written.
constexpr int EIGS_MAX_M = 3 * MG_EIGS_MAX_BLOCK;   // the largest basis [X, W, P]
constexpr int EIGS_TILE = 6;                        // the Gram kernel's tile of (j, l) pairs is EIGS_TILE x EIGS_TILE
// tiles (a, b), a <= b, of an m x m matrix, and the sums one tile leaves: its block of G, then its block of H
inline int eigs_tiles(int m) { const int nt = (m + EIGS_TILE - 1) / EIGS_TILE; return nt * (nt + 1) / 2; }
constexpr int EIGS_TILE_SUMS = 2 * EIGS_TILE * EIGS_TILE;
// blocks of a Gram / a rotation launch over an N x N grid: every sum needs this many partials
size_t eigs_gram_blocks(int N);
size_t eigs_rotate_blocks(int N);
// out[(z*EIGS_TILE_SUMS) + e]: tile z (row-major over a <= b), e = jj*T + ll the entry <S_j, S_l> of G, T*T + jj*T + ll the
// entry <S_j, AS_l> of H (j = a*T + jj, l = b*T + ll; entries with j or l >= m: +0).  ptrs: 2m device pointers, S then AS,
// in device memory; part: eigs_tiles(m)*EIGS_TILE_SUMS*eigs_gram_blocks(N) doubles.  Two launches.
void eigs_gram(hipStream_t s, int N, int m, const double *const *ptrs, double *part, double *out);
// the rotation of include/mg_eigs.h.  ptrs (device memory): EIGS_MAX_M pointers S, EIGS_MAX_M pointers AS (the first m of each
// are read; X' -> S[i], AX' -> AS[i], P' -> S[2p + i], AP' -> AS[2p + i]), then MG_EIGS_MAX_BLOCK pointers R.  coef (device
// memory): C column by column (column i at i*EIGS_MAX_M), Cp likewise from MG_EIGS_MAX_BLOCK*EIGS_MAX_M on, then theta.
// res2[i] = <R_i, R_i>; part: p*eigs_rotate_blocks(N) doubles.  Two launches.
constexpr int EIGS_COEF_CP = MG_EIGS_MAX_BLOCK * EIGS_MAX_M, EIGS_COEF_THETA = 2 * EIGS_COEF_CP,
              EIGS_COEF_COUNT = EIGS_COEF_THETA + MG_EIGS_MAX_BLOCK;
constexpr int EIGS_PTR_AS = EIGS_MAX_M, EIGS_PTR_R = 2 * EIGS_MAX_M, EIGS_PTR_COUNT = 2 * EIGS_MAX_M + MG_EIGS_MAX_BLOCK;
void eigs_rotate(hipStream_t s, int N, int m, int p, double *const *ptrs, const double *coef, double *part, double *res2);
// R_i = AX_i - theta_i*X_i and res2[i] = <R_i, R_i>, i < p: the same tables (S[i], AS[i], R[i], theta).  Two launches.
void eigs_resnorm(hipStream_t s, int N, int p, double *const *ptrs, const double *coef, double *part, double *res2);
// the start of a column: dst = src on the interior (src == nullptr: dst - 0.5, dst holding mg_fill_uniform's values), +0 on the rim
void eigs_start(hipStream_t s, int N, double *dst, const double *src);
}  // namespace k

// residual-tolerance solver pieces shared by mg_solve.cpp and mg_solve_batch.cpp
bool solve_opts_ok(const char *who, int N, double L, const mg_solve_opts &o);
// the constants of one level, formed once at creation in fp64, each operation rounded once and in this order (include/mg_hip.h):
// dx2 = (L/(N-1))^2, inv = 1/dx2, sd = shift*dx2, d = 4 + sd, q = 1/d, c = omega*q -- 4, 0.25 and 0.25*omega exactly at shift = 0
struct LevelConsts {
    double dx2, inv, sd, d, q, c;
    k::Shifted sh;   // {shift != 0, d, q}
};
std::vector<LevelConsts> solve_level_consts(const std::vector<int> &sizes, double L, const mg_solve_opts &o);
// the arrays of one instance's hierarchy, per level (level 0: the caller's F and U, only B[0] is used); the vectors are
// their owner's
struct SolveLevels {
    const std::vector<double *> *A, *B, *F;
    int *gs_state;
    double *gs_err;   // may be nullptr
};
// The operator a hierarchy's levels apply, and with it the kernel family of every operation of the cycle (mg_solve.cpp):
//   kind set               the `_bc` kernels (include/mg_bc.h) with the level's coefficient or nullptr, restrict_bc and
//                          prolong_add_bc with the device tables p_lo / p_w; both norms are resnorm_bc
//     and project_coarse   (include/mg_singular.h: four Neumann sides at shift == 0) the coarse solve is its projecting twin,
//                          gauss_seidel_relative_bc_mean; every other operation is the line above
//   no kind, react set     the `_rx` kernels (include/mg_reaction.h) on (dx2, sd, omega, coef[l] or nullptr, react[l]), with or
//                          without a coefficient; the transfers and the reference norm of the next line, the norm with U is
//                          resnorm_rx.  (A kind and a reaction are never set together: the setters refuse it.)
//   neither of them, coef  the `_vc` kernels (include/mg_varcoef.h) on (dx2, sd, omega, coef[l]), restrict_gather(+1) and prolong
//                          with the cached tables; the norm with U is resnorm_vc, the reference norm ||F|| the constant resnorm
//   none of the three      the constant kernels on cw = lc[l].c and lc[l].sh, the same transfers, resnorm
// Every pointer is its owner's; l is a level of the hierarchy, N = sizes[l].  All members enqueue on st.
struct SolveOperator {
    const mg_solve_opts *o;
    const std::vector<int> *sizes;
    const std::vector<LevelConsts> *lc;
    const int *kind = nullptr;                     // host int[4], S, N, W, E; nullptr: all four sides are Dirichlet
    const std::vector<double *> *coef = nullptr;   // per level: the nodal coefficient; nullptr: a = 1
    const std::vector<int *> *p_lo = nullptr;      // per level l < last: mg_boundary_prolongation_table(sizes[l+1], sizes[l])
    const std::vector<double *> *p_w = nullptr;    // in device memory (read only with kind set)
    bool project_coarse = false;                   // the singular problem (include/mg_singular.h): the coarse solve projects its F
    const std::vector<double *> *react = nullptr;  // per level: the nodal reaction term; nullptr: none (checked before coef)

    const double *a(int l) const { return coef ? (*coef)[l] : nullptr; }
    const double *s(int l) const { return react ? (*react)[l] : nullptr; }
    // one weighted Jacobi sweep in -> out (in == nullptr: from the zero field)
    void sweep(hipStream_t st, int l, const double *in, const double *F, double *out) const;
    // D = -(AU - F)
    void residual(hipStream_t st, int l, const double *U, const double *F, double *D) const;
    // Fc (level l + 1) = the restriction of D (level l)
    void restrict_residual(hipStream_t st, int l, const double *D, double *Fc) const;
    // the relative coarse solve of the last level from zero
    void coarse_solve(hipStream_t st, double *U, const double *F, int *gs_state, double *gs_err) const;
    // Uout (level l) = Uin + P(Uc), Uc of level l + 1
    void prolong_add(hipStream_t st, int l, const double *Uc, const double *Uin, double *Uout) const;
    // *out = ||F - AU|| at level 0 (U == nullptr: the reference norm ||F||); part: resnorm_partials(N) doubles
    void norm(hipStream_t st, const double *U, const double *F, double *part, double *out) const;
    // out = AU at level 0 for the Krylov acceleration, which boundary kinds refuse: apply_rx with a reaction, else apply_vc
    void apply(hipStream_t st, const double *U, double *out) const;
};
// One V(pre, post) cycle as data: its launches in order, each naming the level arrays it reads and writes
// in the five roles of NodeBatchItem.  mg_solver walks it on one instance (run_solve_cycle), mg_batch_solver on its active
// set, one table of NodeBatchItem per slot (mg_solve_batch.cpp).
enum class Field : int { None, U0, F0, A, B, F, Coef };   // U0 / F0: the cycle's own arguments, at its top level
struct FieldRef {
    Field f = Field::None;
    int level = 0;
    bool operator==(const FieldRef &r) const { return f == r.f && level == r.level; }
};
struct SolveStep {
    enum Kind : int { Node, Sweep, Residual, Restrict, Coarse, ProlongAdd, Copy } kind;
    int level;                     // the level the launch runs on (Restrict / ProlongAdd: the fine one)
    int steps = 0, d_sign = 0;     // Node: the sweeps in the launch, and its d_sign
    bool fused_transfer = false;   // Node: carries the restriction (d_sign < 0) or the prolongation-add (d_sign > 0)
    // Sweep: in (None: from zero) -> out on F; Residual: out = -(A in - F); Restrict: out (level + 1) = R in; Coarse: out
    // solved on F from zero; ProlongAdd: out = in + P coarse; Copy: out = in.  coarse of Sweep / Residual / Coarse: the
    // level's coefficient, or None
    FieldRef in, F, coarse, out, Fc;
    int slot = 0;                  // from 1 (table 0 is the norm's); steps whose five roles are equal share one
};
struct SolveCycle {
    std::vector<SolveStep> steps;
    int n_slots = 0;
};
// The cycle over nl levels from level `top` (0: a solve's; above 0: the full-multigrid start), whose iterate U0 keeps its
// guess while coarser levels start from zero, folded into their first sweep.  fused: one Node per level and direction, with
// the transfer inside where down_fused[l] / up_fused[l] (read only then), beside it elsewhere; else operator by operator,
// one Sweep per launch.  with_coef: Sweep, Residual and Coarse name Coef[level].  Every field choice of the cycle is made
// here; touches no table and no device.
SolveCycle build_solve_cycle(int nl, int pre, int post, int top, bool fused, const int *down_fused, const int *up_fused, bool with_coef);
// whether the streaming node of level l < last carries its restriction / its prolongation-add (the builder's inputs)
void solve_fusable_levels(const std::vector<int> &sizes, std::vector<int> *down_fused, std::vector<int> *up_fused);
// a Node step as the streaming launcher takes it, on the arrays `it` (a batched launch adds .batch)
k::SmoothNode<double> solve_cycle_node(const SolveStep &s, const std::vector<int> &sizes, const std::vector<LevelConsts> &lc,
                                       const NodeBatchItem &it);
// enqueue the cycle on one instance with the kernels of op (a Node: the constant operator's streaming smoother); returns the
// kernel launches (the final copy is none).  F0, U0: of the size of the cycle's top level
int run_solve_cycle(hipStream_t st, const SolveCycle &c, const SolveLevels &lv, const SolveOperator &op, const double *F0, double *U0);
// the level-0 coefficient of a solver, mg_solver::coef[0] (mg_solve.cpp), nullptr when none is set: the heat stepper's
// right-hand-side kernel reads the solver's own array instead of keeping a second copy (mg_heat.cpp)
const double *solver_coefficient(const mg_solver *s);
// the four kinds of a solver (mg_solver::bc, S, N, W, E), nullptr when every side is Dirichlet
const int *solver_boundary(const mg_solver *s);
// what a driver over the solvers needs of their shape (mg_adjoint.cpp): N, and L / max_batch where asked for
int solver_size(const mg_solver *s, double *L);
int batch_solver_size(const mg_batch_solver *s, double *L, int *max_batch);
// the level-0 coefficient instance i of a batched solve uses (mg_solve_batch.cpp): its own copy, the shared one, or nullptr
// when none is set
const double *batch_solver_coefficient(const mg_batch_solver *s, int i);
// one cycle of a batch solver's own, U0[i] = vcycle(F0[i], U0[i]) for i < n <= max_batch, as an iteration of
// mg_batch_solver_solve enqueues it (the constant, the variable-coefficient or, under MG_SMOOTHER=simple, the operator-by-
// operator cycle) -- for a driver that uses the cycle as a preconditioner (mg_eigs.cpp).  Rebuilds and uploads the solver's
// tables; returns the launches it enqueued, or -1 on a HIP error.
int batch_solver_cycle(mg_batch_solver *s, hipStream_t st, int n, const double *const *F0, double *const *U0);
// the coarse solves' state of that cycle: enqueue its copy into the solver's pinned block behind the cycle (no synchronisation);
// once the stream has been synchronised, whether a coarse solve of the instances 0 .. n-1 stopped at coarse_max_iters
bool batch_solver_enqueue_state(mg_batch_solver *s, hipStream_t st);
bool batch_solver_coarse_capped(const mg_batch_solver *s, int n);

// The pre-smoothed U of a level is dead weight between its `-1` and its `1` node: 8 B per point written, 8 B read.  When
// recompute_available(), the `-1` node (zero start) may run with smooth_restrict_no_out() and the `1` node with
// prolong_smooth_recompute(), which redoes the `pre` sweeps from zero on the same F inside its own pipeline: the same
// expressions, the same bits, two array passes less.
bool recompute_available(int Nc, int N, int pre, int step);
int  recompute_min_n();   // MG_RECOMPUTE_MIN_N (default 4096)
// launch a recorded fused node on n instances (batch == nullptr: on the arrays recorded in op itself)
void replay_node(const NodeOp &op, const NodeBatch *batch);
void smooth_restrict_no_out(int N, double L, double *U_unused, double *F, int step, double *error_dev, int M, double *F_c);
void prolong_smooth_recompute(int Nc, const double *U_c, int N, double L, double *U_out, double *F, int pre, int step, double *error_dev);
// the same pair on fp32 fields (mixed-precision mode); U_out_wide != nullptr: the result is stored in fp64 there
void smooth_restrict_f32_no_out(int N, double L, float *U_unused, float *F, int step, double *error_dev, int M, float *F_c);
void prolong_smooth_f32_recompute(int Nc, const float *U_c, int N, double L, float *U_out, double *U_out_wide, const float *F, int pre,
                                  int step, double *error_dev);
// mg_prolong_smooth_f32 whose result goes to an fp64 array (exact widening in the store) instead of U_out
void prolong_smooth_f32_wide(int Nc, const float *U_c, int N, double L, const float *U_in, double *U_out_wide, const float *F,
                             int step, double *error_dev);
// fp32 view of a coarse-tail slice: spacings and transfer weights rounded once (mg_cycle.cpp)
k::TailArgsF tail_args_f32(const k::TailArgs &a);
// collect the coarse-tail slice of a cycle file's node stream (mg_cycle.cpp)
bool scan_tail(const std::vector<double> &tokens, size_t *tok_io, const std::vector<int> &sizes, int at0, int con_step,
               int top_N, double L, k::TailArgs *out, int *node_level);

// the adjoint of reaction and semilinear solves (mg_adjoint_rx_kernels.hip, driven by mg_adjoint_rx.cpp; the expressions and
// their order: include/mg_adjoint_rx.h).  G = kappa*(lam'*g(U)) on the interior and +0 on the rim, *out = the sum of
// W*(lam'*g(U)) (W == nullptr: of lam'*g(U)) in the partition and order of the semilinear pass's norm, no square root
// (part: resnorm_partials(N)).  kind: MG_NEWTON_* or MG_GRAD_LINEAR.  Two launches.
namespace k {
void src_grad(hipStream_t s, int N, int kind, double kappa, const double *W, const double *lam, const double *U, double *G, double *part,
              double *out);
// the same on n instances in one launch and one finish launch: items[z] the arrays and the kappa of instance z; has_w: EVERY
// instance's W is there (false: the slot is not read).  Partials at part + z*resnorm_partials(N), sums to out[z].
struct SrcGradItem {
    const double *W, *lam, *U;
    double *G;
    double kappa;
};
void src_grad_batch(hipStream_t s, int n, int N, int kind, bool has_w, const SrcGradItem *items, double *part, double *out);
}  // namespace k
// The linearisation of the semilinear problem at U for a driver outside mg_solve.cpp (mg_adjoint_rx.cpp): refuses what
// mg_solver_newton refuses (messages under `who`), checks w, runs the no-step pass on U -- S into the solver's level-0
// reaction storage, *res = ||N(U)|| -- coarsens S as mg_solver_newton does and leaves the solver WITH that reaction.  Returns
// MG_OK, or the error code with the solver without a reaction.  solver_drop_reaction: the solver without a reaction again.
int solver_newton_linearise(mg_solver *s, const char *who, int kind, double kappa, const double *w_dev, const double *F_dev,
                            const double *U_dev, double *res);
void solver_drop_reaction(mg_solver *s);
// the same for n instances of a batch solver (mg_solve_batch.cpp): what mg_batch_solver_newton refuses, ONE pass over all n --
// S of instance i straight into its level-0 reaction storage, norms[i] = ||N(U_i)|| (host, may be nullptr) -- and one coarsening
// launch per level; leaves the solver with n reaction terms, one per instance.  *launches grows by the kernel launches.
int batch_solver_newton_linearise(mg_batch_solver *s, const char *who, int n, int kind, const double *kappa, int n_w,
                                  const double *const *w_dev, const double *const *F_dev, const double *const *U_dev, double *norms,
                                  int *launches);
void batch_solver_drop_reaction(mg_batch_solver *s);

}  // namespace mg
