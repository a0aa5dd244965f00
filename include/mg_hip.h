/*
 * mg_hip.h -- C ABI of the MI355X-native multigrid Poisson engine (libmgpoisson.so).
 *
 * Drop-in boundary for the V/W-cycle hot path of cindytsai/multigrid_poisson_solver.
 * The reference has no FFI layer: its "interface" is the set of free functions its
 * driver calls (src/MG_solver_CPU.cpp:16-30, GPU twins src/MG_solver_GPU.cu:27-41).
 * Every operator below keeps the reference's argument list and meaning; the one
 * change is that U/F/D are DEVICE-resident fp64 arrays (row-major N x N,
 * index = col + N*row, boundary included -- src/MG_solver_CPU.cpp:484) obtained from
 * mg_alloc(), because re-uploading per call (src/MG_solver_GPU.cu:1159-1282) can never
 * approach the HBM roofline.  include/mg_dropin.hpp maps the reference's C++ names
 * onto these symbols so the reference's own main() compiles against this library
 * (see INTEGRATION.md).
 *
 * Conventions kept from the reference: caller owns all arrays,
 * callee may use internal scratch, results are visible when the call returns for every
 * entry point that hands a value back to the host, single caller thread, int sizes.
 * Errors: the reference printf+exit(1)s; here a failed call prints to stderr, records
 * a code readable through mg_last_error() and (default) aborts the process with
 * exit(1) -- mg_set_abort_on_error(0) turns the abort off for embedding in tests.
 *
 * All calls are enqueued on ONE HIP stream (mg_set_stream / mg_get_stream).
 */
#ifndef MG_HIP_H
#define MG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* lifecycle                                                                  */
/* ------------------------------------------------------------------------- */
/* replaces cudaSetDevice(0), src/MG_solver_GPU.cu:58-62.  Returns 0 on success. */
int         mg_init(int device);
void        mg_finalize(void);
/* use the caller's hipStream_t (NULL = the engine's own stream) */
void        mg_set_stream(void *hip_stream);
void       *mg_get_stream(void);
void        mg_sync(void);
int         mg_last_error(void);
const char *mg_last_error_string(void);
void        mg_clear_error(void);
void        mg_set_abort_on_error(int on);
/* "stream" (default: temporally blocked wave-streaming kernels) or "simple"
 * (one launch per sweep, one thread per point); also read from env MG_SMOOTHER. */
int         mg_set_smoother(const char *name);
const char *mg_version(void);

/* ------------------------------------------------------------------------- */
/* memory: replaces malloc/free of ListNode (src/linkedlist.cpp:9-11,21-23,48-50)
 * and of tempU (src/MG_solver_CPU.cpp:353,371).  Served from a caching pool so the
 * timed window contains no hipMalloc.                                         */
/* ------------------------------------------------------------------------- */
double *mg_alloc(size_t n_doubles);
void    mg_free(double *dev);
void    mg_pool_trim(void);
size_t  mg_pool_bytes(void);
void    mg_upload(double *dev, const double *host, size_t n_doubles);   /* synchronous */
void    mg_download(double *host, const double *dev, size_t n_doubles); /* synchronous */
/* Memory contract of every entry point that takes a device array (tests/test_memory_contract_gpu.py holds each call to
 * it inside guard bands): a call writes the arrays it is documented to write and nothing else -- not one byte before or
 * after them -- and only reads the others.  `const` arguments are read only; for the non-const pointers of the drop-in
 * signatures the comment at the prototype says which are read only.  The one input a call may overwrite is U_in of
 * mg_smooth_pp.  Arrays need the alignment of mg_alloc's blocks at most (16 bytes is what the solvers demand). */
void    mg_copy(double *dst_dev, const double *src_dev, size_t n_doubles);
/* memset(U, 0, N*N*8): src/MG_solver_CPU.cpp:213,256 */
void    mg_fill_zero(double *dev, size_t n_doubles);
/* D[i] = -D[i] (in place) for all N*N entries: the driver's own loop, src/MG_solver_CPU.cpp:277-280 */
void    mg_negate(int N, double *D);

/* ------------------------------------------------------------------------- */
/* problem definition: src/MG_solver_CPU.cpp:468-548                          */
/* ------------------------------------------------------------------------- */
void mg_getSource(int N, double L, double *F, double min_x, double min_y);
/* where mg_getSource (and the drivers' own getSource at load, :153) evaluates F:
 * "auto" (default): on the device (k_source: no host pass, no PCIe) when that reproduces THIS host's libm bit for
 *   bit -- the reference calls libm's exp() (:488), and the device evaluates glibc's algorithm for it (table +
 *   polynomial, FMA form); the engine compares the two on ~130k points once per process (mg_source_is_bit_identical)
 *   and falls back to "host" when they differ (another libm, a CPU without FMA), and per call for grids whose
 *   arguments x - y leave the verified main path of the algorithm (|min_x - min_y| + |L| >= 511: glibc's overflow
 *   and subnormal special cases are not reproduced on the device).  mg_getAnalytic / mg_analyticError always use the
 *   device form: outside that range their exp() is the device's own (<= 1 ulp from libm's);
 * "host": libm on the host cores, chunked through 2 x 128 MiB of pinned staging;
 * "device": the device form unconditionally.  Also env MG_SOURCE. */
int  mg_set_source(const char *mode);
/* "host" or "device": what mg_getSource will use (runs the check in auto mode) */
const char *mg_source_mode(void);
int  mg_source_is_bit_identical(void);
void mg_getAnalytic(int N, double L, double *U, double min_x, double min_y);
/* sum|analytic - U| / (N*N): src/MG_solver_CPU.cpp:434-445; result to *error_host */
void mg_analyticError(int N, double L, const double *U, double min_x, double min_y, double *error_host);

/* ------------------------------------------------------------------------- */
/* the six operators: src/MG_solver_CPU.cpp:23-28 (same order, same arguments)  */
/* ------------------------------------------------------------------------- */
/* :554-564.  U and F are read only; every element of D is written (the rim: zero) */
void mg_getResidual(int N, double L, double *U, double *F, double *D);
/* :566-571: U1 += U2.  U2 is read only */
void mg_doGridAddition(int N, double *U1, double *U2);
/* :573-625.  error is a HOST pointer (as in the reference, where it points into the
 * ListNode); the call returns after the value is written.  NULL = not wanted.  U is smoothed in place, F is read only. */
void mg_doSmoothing(int N, double L, double *U, double *F, int step, double *error);
/* :627-638, option 1 = red-black Gauss-Seidel :952-1066.  option 0 (dense inverse) is
 * refused with the message of src/MG_solver_GPU.cu:1286-1289.  U is written (whatever it held is ignored: the solve starts
 * from zero), F is read only. */
void mg_doExactSolver(int N, double L, double *U, double *F, double target_error, int option);
/* :640-680.  U_f is read only; every element of U_c is written */
void mg_doRestriction(int N, double *U_f, int M, double *U_c);
/* :682-724.  U_c is read only; the points of U_f that no coarse cell owns keep their values */
void mg_doProlongation(int N, double *U_c, int M, double *U_f);

/* ------------------------------------------------------------------------- */
/* asynchronous / fused forms used by the engine's own driver                 */
/* ------------------------------------------------------------------------- */
/* step Jacobi sweeps from U_in into U_out (U_out != U_in; U_in is clobbered as
 * scratch when more than one launch is needed).  U_in == NULL means "U is all zero"
 * (the driver's memset of src/MG_solver_CPU.cpp:256 folded into the first sweep).
 * error_dev (device pointer or NULL) receives doSmoothing's error; D_out (device
 * pointer or NULL) receives getResidual(U_out) times d_sign (+1 or -1: the driver's
 * sign flip :277-280 folded in).  F is read only. */
void mg_smooth_pp(int N, double L, const double *U_in, double *U_out, double *F, int step,
                  double *error_dev, double *D_out, int d_sign);
/* one "-1" node of the driver (:259-287): U_out = smooth^step(U_in or 0), then
 * F_c = doRestriction(N, -getResidual(U_out), M) -- one pass over HBM when fusable.  U_in and F are read only (when
 * several launches are needed the partner of U_out is engine scratch, not U_in). */
void mg_smooth_restrict(int N, double L, const double *U_in, double *U_out, double *F, int step,
                        double *error_dev, int M, double *F_c);
/* one "1" node of the driver (:353-416): U_out = smooth^step(U_in + doProlongation(Nc, U_c, N)).  U_c, U_in and F are
 * read only. */
void mg_prolong_smooth(int Nc, const double *U_c, int N, double L, const double *U_in, double *U_out,
                       double *F, int step, double *error_dev);
/* mixed-precision mode (README.md:269-270 of the reference: "single
 * precision" GPU kernels): the two fused nodes with every array and every arithmetic operation
 * in fp32 (norms in fp64).  Zero start only for the "-1" node; 1..4 steps.  Even N with a nested
 * coarse size runs as ONE launch, anything else operator by operator (same results).  F (and U_c, U_in) are read only. */
void   mg_smooth_restrict_f32(int N, double L, const float *U_in, float *U_out, float *F, int step,
                              double *error_dev, int M, float *F_c);
void   mg_prolong_smooth_f32(int Nc, const float *U_c, int N, double L, const float *U_in, float *U_out,
                             float *F, int step, double *error_dev);
float *mg_alloc_f32(size_t n_floats);
void   mg_free_f32(float *dev);
void   mg_to_f32(float *dst_dev, const double *src_dev, size_t n);   /* round to nearest */
void   mg_to_f64(double *dst_dev, const float *src_dev, size_t n);   /* exact */
void   mg_upload_f32(float *dev, const float *host, size_t n);       /* synchronous */
void   mg_download_f32(float *host, const float *dev, size_t n);     /* synchronous */
/* U_f_out = U_f_in + doProlongation(N, U_c, M) in one pass (:354 + :368) */
void mg_prolongAdd(int N, const double *U_c, int M, const double *U_f_in, double *U_f_out);
/* doRestriction(N, sign*U_f, M, U_c) */
void mg_restrict_signed(int N, const double *U_f, int M, double *U_c, int sign);
/* number of Gauss-Seidel iterations the last mg_doExactSolver call ran (synchronises) */
int  mg_lastExactSolverIterations(void);

/* ------------------------------------------------------------------------- */
/* host-side index tables (exact reference expressions, fp64 on the host)      */
/* ------------------------------------------------------------------------- */
/* doRestriction :661-666: lo[i] = (int)floor(i*h_c/h_f), w[i] = fmod(i*h_c,h_f)/h_f */
void mg_restriction_table(int N, int M, int *lo, double *w);
/* doProlongation :697-718: owner of fine index k along rows (axis 0) or columns
 * (axis 1) and the two 1-D weights (c_hi - f, f - c_lo) the kernel multiplies with */
void mg_prolongation_table(int N, int M, int axis, int *owner, double *w_hi, double *w_lo);

/* ------------------------------------------------------------------------- */
/* synthetic inputs and checksums (benchmark + full-size parity tests)         */
/* ------------------------------------------------------------------------- */
/* dst[i] = uniform[0,1) from a counter-based 64-bit hash of (i + seed); the same
 * recipe as tests/_synth.py:hash_uniform */
void mg_fill_uniform(double *dst, size_t n_doubles, uint64_t seed);
/* out[0] = sum of bit patterns, out[1] = sum of bit patterns * (2*i+1), mod 2^64,
 * with -0.0 canonicalised to +0.0 (tests/_synth.py:checksum); synchronous */
void mg_checksum(const double *src, size_t n_doubles, uint64_t out[2]);

/* ------------------------------------------------------------------------- */
/* live kernel timing (bench.py's roofline object): hipEvent pairs recorded on   */
/* the engine's stream around every operator launch on grids with N >= min_N     */
/* ------------------------------------------------------------------------- */
typedef struct mg_profile_entry {
    char   name[64];        /* kernel family, e.g. "jacobi_stream<3>" */
    int    N;               /* grid size */
    int    launches;
    double total_ms;        /* sum of the launches' durations */
    double algo_bytes;      /* ALGORITHMIC bytes of ONE launch */
} mg_profile_entry;
void mg_profile_begin(int min_N);
/* time the launches of every `every`-th cycle window (mg_cycle_enqueue) only -- the 1st, the (every+1)-th, ...; 1 = all */
void mg_profile_sample(int every);
/* synchronises, fills out[0..cap) with one entry per (name, N), returns the count */
int  mg_profile_end(mg_profile_entry *out, int cap);

/* ------------------------------------------------------------------------- */
/* geometry record of the streaming smoother (host side only, off by default)  */
/* ------------------------------------------------------------------------- */
/* While the log is on, every launch of the streaming kernel appends one record when it is ENQUEUED (a traced, batched
 * or graph-captured plan records while it is built, not when it replays).  A record is MG_STREAM_GEOMETRY_FIELDS ints:
 *   N, own rows (N, or the rows of a slab window), rows_per_chunk, chunks, groups (workgroups per chunk row),
 *   instances (of a batch, else 1), S (sweeps), COLS (columns per lane), IN (0 load, 1 zero, 2 prolong), RESTRICT,
 *   PRE (recomputed pre-sweeps), flags (MG_GEOMETRY_NT | _WT | _SH | _F32).
 * The chunk height is the launcher's choice (device, occupancy, batch size, slab window, env MG_RESIDENT_PCT,
 * MG_MAX_ROWS); no result depends on it.  The log keeps at most 65536 records: later ones are dropped, and the next
 * fetch reports that as an error (MG_ERR_ARG). */
#define MG_STREAM_GEOMETRY_FIELDS 12
#define MG_GEOMETRY_NT  1   /* non-temporal stores of U */
#define MG_GEOMETRY_WT  2   /* weighted sweep */
#define MG_GEOMETRY_SH  4   /* screened (shifted) operator */
#define MG_GEOMETRY_F32 8   /* fp32 fields */
/* on != 0: start recording (the log is emptied); 0: stop and empty it */
void mg_stream_geometry_log(int on);
/* copies the oldest records, at most cap of them, to out (MG_STREAM_GEOMETRY_FIELDS ints each) and removes them from
 * the log; returns how many.  out == NULL: the number of records waiting, nothing removed. */
int  mg_stream_geometry_fetch(int *out, int cap);

/* ------------------------------------------------------------------------- */
/* cycle-file driver: main() of src/MG_solver_CPU.cpp:36-462                   */
/* ------------------------------------------------------------------------- */
typedef struct mg_node_record {
    int    node;   /* -1, 0, 1 */
    int    N;
    int    steps;
    double error;
} mg_node_record;

typedef struct mg_cycle_result {
    int     status;        /* 0 ok */
    int     N;             /* finest grid */
    double *U_dev;         /* final solution (device, owned by the plan) */
    double  mg_error;      /* :434-445 */
    double  time_ms;       /* host wall clock of the reference's window :156..:429, synchronised */
    double  device_ms;     /* hipEvent time of the last window.  A window enqueued on an idle stream: from its own start
                            * event to its end event, as mg_cycle_execute's.  A window enqueued while the previous window
                            * of this plan was still running or waiting (back to back): from the END of that window to the
                            * end of this one -- the boundary between the two is included, and so is anything else the
                            * caller put on the stream in between.  The decision is taken once, with hipEventQuery when the
                            * window is enqueued: should the previous window finish after that query but before this
                            * window's first launch reaches the device (a host slower than the device, small grids), the
                            * idle time in between is counted too.  0 for a window enqueued inside a stream capture. */
    int     n_records;
    const mg_node_record *records; /* owned by the plan, valid until the next execute */
    const char *report;    /* the reference's printed report (owned by the plan) */
    int     graph_replayed;     /* 1: the last window was a hipGraph replay (MG_CYCLE_GRAPH took effect), 0: launched eagerly */
    int     schedule_launches;  /* > 0: the window ran as a batched breadth-first schedule of this many launches (the
                                 * independent visits of a level merged into one launch each); 0: node by node */
} mg_cycle_result;

typedef struct mg_cycle_plan mg_cycle_plan;

#define MG_CYCLE_FUSED   1 /* use the fused operators (default driver mode) */
#define MG_CYCLE_GRAPH   2 /* capture the node program into a hipGraph and replay it */
#define MG_CYCLE_REPORT  4 /* build the printed report text */
#define MG_CYCLE_ERROR   8 /* evaluate mg_error (:434-445) after the window, as the program does */
#define MG_CYCLE_MIXED  16 /* the whole cycle in fp32 (F rounded once at load, U widened at the end);
                              fixed-step halving files whose coarse part fits the tail kernel */

/* parse a cycle structure file (README.md:43-128); allocates the finest level and
 * evaluates getSource on it (:149-153, outside the timed window) */
mg_cycle_plan *mg_cycle_load(const char *path, int flags);
/* one run of the reference's timed window from the state right after getSource */
int            mg_cycle_execute(mg_cycle_plan *plan, mg_cycle_result *out);
/* the same window without host synchronisation: enqueue any number back to back, then collect
 * (waits, reports the last one).  mg_cycle_execute == sync + enqueue + sync + collect.
 * A window leaves its smoothing errors as partial sums in the plan's own memory; mg_cycle_collect reduces those of the
 * last window (one launch per collect, none per window: the errors of earlier windows are never reported).  Trigger mode
 * (con_step = -1) reduces at the end of its window.  A back-to-back window records one timing event, not two: device_ms. */
int            mg_cycle_enqueue(mg_cycle_plan *plan);
int            mg_cycle_collect(mg_cycle_plan *plan, mg_cycle_result *out);
/* MG_CYCLE_MIXED plans: `cycles` fp32 runs of the file per window, joined by the fp64 residual of
 * the fp64 iterate and an fp64 correction (iterative refinement; BASELINE.json configs[4]).  The
 * errors are doSmoothing's metric (src/MG_solver_CPU.cpp:607-622) of the iterate after 1 .. cycles-1
 * corrections. */
int            mg_cycle_set_refinement(mg_cycle_plan *plan, int cycles);
int            mg_cycle_refinement_errors(mg_cycle_plan *plan, double *out, int cap);
void           mg_cycle_destroy(mg_cycle_plan *plan);
/* the whole reference program: load, execute, print report, write Sol_HIP_<file> CSV */
int            mg_cycle_main(int argc, char **argv);
/* CSV writer of src/MG_solver_CPU.cpp:735-754 on a device array */
int            mg_print2File(int N, const double *U_dev, const char *file_name);

/* ------------------------------------------------------------------------- */
/* 1-D row-slab decomposition over the GPUs of one node (no reference            */
/* counterpart: the reference is single-device, src/MG_solver_GPU.cu:58)         */
/* ------------------------------------------------------------------------- */
/* RCCL communicator, one process per GPU.  Rank 0 creates the id, the caller ships its
 * mg_comm_unique_id_bytes() bytes to every rank (e.g. torch.distributed broadcast). */
int  mg_comm_unique_id_bytes(void);
int  mg_comm_get_unique_id(void *out);
int  mg_comm_init(int rank, int nranks, const void *unique_id);
/* Host-staged transport instead of RCCL: the slab driver's ghost-row groups and its all-gather are
 * handed to two callbacks of the embedding program (MPI, gloo, ...) with HOST buffers.  `exchange`
 * receives the n_ops point-to-point operations of one group (is_send[i], peer[i], buf[i],
 * bytes[i]) and returns 0 when ALL of them have completed; operations between two ranks
 * are posted in the same order on both sides.  `allgather` fills recv[r*count .. ] with rank r's
 * `send`.  Purpose: running the real rank-mode driver with several processes on one GPU (RCCL
 * allows one rank per device), and clusters without xGMI.  Arithmetic stays on the device. */
typedef struct mg_host_transport {
    void *user;
    int (*exchange)(void *user, int n_ops, const int *is_send, const int *peer, void *const *buf, const size_t *bytes);
    int (*allgather)(void *user, const double *send, double *recv, size_t count_per_rank);
} mg_host_transport;
int  mg_comm_init_host(int rank, int nranks, const mg_host_transport *transport);
/* exercises the RCCL calls of the slab driver (grouped send/recv on a second stream ordered by events, all-gather)
 * against this rank itself and checks the bytes; 0 = ok.  Runs with a 1-rank communicator on a one-GPU box. */
int  mg_comm_selftest(size_t n_doubles);
void mg_comm_finalize(void);
int  mg_comm_rank(void);
int  mg_comm_size(void);
/* the shared object the RCCL entry points in use were resolved from (absolute path as the loader mapped it), "host
 * transport ..." after mg_comm_init_host, "" before any communicator exists: lets a benchmark record prove which wire
 * and how many ranks (mg_comm_size) it ran on */
const char *mg_comm_library(void);

/* host-only: row ranges per level and rank of the hierarchy N_max, N_max/2, ... >= N_min.
 * out[(level*nranks + rank)*2 + {0,1}] = [lo, hi); collapsed_out[level] = 1 where the level
 * is collapsed (replicated whole on every rank; reported as [0, N) for rank 0 and [0, 0) for the
 * others).  Returns the number of levels. */
int  mg_slab_partition(int N_max, int N_min, int nranks, int collapse_N, int *out, int *collapsed_out);
/* a level stays distributed while every slab keeps at least 2 * mg_slab_ghost_rows() rows */
int  mg_slab_ghost_rows(void);
/* host-only: the communication-avoiding schedule mg_slab_load derives for a hierarchy (`steps` sweeps per node).
 * Per distributed level and rank: own = owned rows; dext = rows its `-1` launch updates (owned rows + the rows whose
 * restricted residual is the next level's F halo, recomputed instead of exchanged); ext = rows its `1` launch updates
 * (owned rows + what the next finer level's prolongation reads); fwr = rows of the level's F the finer level's launch
 * writes.  Per level: halo rows per side, needF (F rows read beyond the owned ones), xF / xU (rows of the level's F /
 * U halo that DO travel: xF on the critical path right after the finer level's `-1` launch, xU on a second stream,
 * needed only when the cycle comes back up through the level).
 *   ca_mode 0: exchange every halo (one group per level); 1 (default): recompute F halos while the extra rows stay
 *   below ca_pct per cent of a slab (default 10); 2: recompute U halos too.  Negative = env MG_SLAB_CA / MG_SLAB_CA_PCT.
 * level_out[l*6 ..] = {N, collapsed, halo, needF, xF, xU}; rank_out[(l*nranks + r)*8 ..] = {own, dext, ext, fwr} as
 * [lo, hi) pairs.  Returns the number of levels, -1 when a halo would not fit the neighbouring slab. */
int  mg_slab_schedule(int N_max, int N_min, int nranks, int collapse_N, int steps, int ca_mode, int ca_pct,
                      int *level_out, int *rank_out);
/* host-only: pre_out[l] > 0 = on level l (only distributed levels matter) the `-1` launch does not store the smoothed
 * U and the `1` launch recomputes it, pre_out[l] sweeps from zero on F, instead of reading it (fp64 plans, levels of
 * at least MG_RECOMPUTE_MIN_N = 4096 points per side; MG_SLAB_RECOMPUTE=0 switches it off): such a level has no U
 * halo.  Returns the number of levels. */
int  mg_slab_recompute_levels(int N_max, int N_min, int steps, int *pre_out);
/* the same for a plan of `nranks` slabs: what decides is the size of a launch -- N * (N / nranks) >= MG_RECOMPUTE_MIN_N^2 / 2
 * points -- so the smaller distributed levels of a many-rank plan store and re-read their U (and exchange its halo) */
int  mg_slab_recompute_levels_ranks(int N_max, int N_min, int steps, int nranks, int *pre_out);
/* host-only: 1 when this build holds the recomputing fused `1` node for `pre` pre-smoothing + `post` post-smoothing
 * sweeps (1+1, 2+2, 3+3 in the default build; none in a build with another prefetch depth): the node pair that
 * neither stores nor re-reads a level's pre-smoothed U (src/MG_solver_CPU.cpp:259 ... :416 of one level).  Other
 * sweep counts -- and cycle files with per-node step counts, con_step = 0 -- run the store/re-read form. */
int  mg_recompute_pair_available(int pre, int post);

typedef struct mg_slab_plan mg_slab_plan;
/* rank >= 0: this process is that rank (needs mg_comm_init when nranks > 1).  rank == -1:
 * all nranks slabs live in this process and exchange by device copies ("virtual ranks":
 * how the decomposition is verified bit for bit on one GPU).  Levels with N <= collapse_N
 * are replicated: every rank runs them on the whole grid.  Supported grammar: con_N = 1, fixed con_step in 1..4, option 1. */
mg_slab_plan *mg_slab_load(const char *path, int nranks, int rank, int collapse_N);
/* the same with flags: MG_CYCLE_MIXED = the whole cycle on fp32 slabs (half the HBM and xGMI bytes;
 * source rounded once, exact solver in fp64, mg_slab_gather_U widens), BASELINE.json configs[4] */
mg_slab_plan *mg_slab_load_flags(const char *path, int nranks, int rank, int collapse_N, int flags);
/* MG_CYCLE_MIXED slab plans: like mg_cycle_set_refinement / mg_cycle_refinement_errors.  Each extra cycle
 * costs one ghost exchange of the fp64 iterate and one of the new fp32 source on the finest level. */
int  mg_slab_set_refinement(mg_slab_plan *plan, int cycles);
int  mg_slab_refinement_errors(mg_slab_plan *plan, double *out, int cap);
/* one run of the reference's timed window; U_dev is NULL (use mg_slab_gather_U) */
int  mg_slab_execute(mg_slab_plan *plan, mg_cycle_result *out);
/* like mg_cycle_enqueue / mg_cycle_collect */
int  mg_slab_enqueue(mg_slab_plan *plan);
int  mg_slab_collect(mg_slab_plan *plan, mg_cycle_result *out);
/* owned rows of this process's slabs of the finest U into a full N x N host array */
int  mg_slab_gather_U(mg_slab_plan *plan, double *host_full);
/* mg_error (src/MG_solver_CPU.cpp:434-445) is evaluated after each window unless turned off */
void mg_slab_want_error(mg_slab_plan *plan, int on);
void mg_slab_destroy(mg_slab_plan *plan);

/* ------------------------------------------------------------------------- */
/* residual-tolerance solver: V(pre, post) cycles on a caller's F and boundary    */
/* until ||F - AU||_2 <= max(rtol*||F||_2, atol) over the interior points         */
/* ------------------------------------------------------------------------- */
/* Hierarchy: N, N/2, ... while >= N_min (the sizes mg_cycle_load derives for a header `N N_min` with con_N = 1);
 * N_min in [3, 32], at least two levels (N >= 2*N_min).  One cycle is the reference driver's V(pre, post) node order
 * (src/MG_solver_CPU.cpp:259-416) started from the caller's U (the finest level keeps its guess, :252-257; coarser
 * levels start from zero) with two changes: the smoother is weighted Jacobi, U <- U + c*t with t the reference's bracket
 * star - 4U - dx^2 F and c = 0.25*omega (product and sum rounded separately; omega = 1 is doSmoothing bit for bit), and
 * the coarsest level runs the reference's red-black Gauss-Seidel from zero until err <= max(coarse_atol,
 * coarse_rtol*err0), err0 = sum_interior|F| / (N-2)^2, at most coarse_max_iters iterations (coarse_rtol = 0 with
 * coarse_atol = tol is the reference's exact solve).  Residual, restriction, prolongation, addition and the sign flip
 * are the reference operators.  U (in/out): initial guess whose rim carries the Dirichlet values; the rim of F is
 * ignored.  On N = 2^k and 2^k + 1 hierarchies the rim comes back bit-identical; on other sizes the reference's
 * prolongation may move rim points by rounding (about 1e-14 seen).
 * shift (sigma >= 0, finite) makes it the screened equation  Laplace(U) - sigma*U = F  on every level (coarse levels are
 * rediscretised with the same sigma): the equation of an implicit time step, sigma = 1/(nu*dt), F = -u_old/(nu*dt).
 * Per level of size N_l the host forms in fp64, each operation rounded once, dx2 = (L/(N_l-1))^2, inv = 1/dx2,
 * d = 4 + shift*dx2, q = 1/d, c = omega*q (4, 0.25, 0.25*omega at shift = 0).  Bracket b(U) = (((U[r+1] + U[r-1]) +
 * U[c+1]) + U[c-1]) - d*U with the product rounded before the subtraction; sweep U <- U + c*(b(U) - dx2*F); residual (the
 * restricted quantity and the stopping norm) inv*b(U) - F; coarse update q*(left + right + down + up - dx2*F) with error
 * metric sum|inv*b(U) - F| / (N-2)^2.  The transfer operators, the tolerances and the results keep their definitions.
 * shift = 0 is the Poisson solve above bit for bit, through the same kernels; a negative shift (the indefinite Helmholtz
 * problem) is refused with MG_ERR_ARG.
 * ABI: `shift` was appended to mg_solve_opts in version 0.2; a caller compiled against the 0.1 header passes a shorter
 * struct and must be recompiled (mg_version() tells the two apart).
 *
 * fmg (full-multigrid start; 0 = none: everything above, bit for bit, through the same launches; n in 1..8 = n V-cycles
 * per coarse level during the ascent; anything else is refused with MG_ERR_ARG).  With fmg >= 1 a solve whose start does
 * not already meet the tolerance first replaces the INTERIOR of U by the FMG guess -- the interior the caller passed is
 * ignored, the rim is the Dirichlet data and is not written by the pass -- and then runs the cycle loop above.  history[0]
 * and res0 stay the norm of the caller's start, the pass is not counted in `cycles` (with max_cycles = 0 the pass still runs
 * and res stays res0); a start that meets the tolerance runs nothing and leaves U untouched.  Levels l = 0 (finest) ..
 * last are the hierarchy's sizes N_l.  The pass:
 *  1. F_0 = F, F_{l+1} = doRestriction(N_l, F_l, N_{l+1}).
 *  2. Rim data g_0 = the rim of U (four edges: row 0, row N-1, column 0, column N-1); each edge of g_{l+1} is the edge of
 *     g_l sampled at the N_{l+1} coarse points with the 1-D table mg_cubic_table(N_l -> N_{l+1}) (mg_fmg.h) in the order
 *     ((w0*s0 + w1*s1) + w2*s2) + w3*s3, corners included (they are end points of the edges: t = 0 and t = N_l - 1).
 *  3. Coarsest level: r = -getResidual(rim_only(g_last), F_last) (the field with g_last on its rim and +0 inside; with
 *     shift, the screened residual), e = the coarse solve of A e = r from zero with coarse_rtol / coarse_atol /
 *     coarse_max_iters as in a cycle (it reads no rim value of r), u_last = e inside, g_last on the rim.
 *  4. For l = last-1 .. 0: the interior of u_l = mg_prolongCubic(u_{l+1}) (rim included as data), the rim of u_l = g_l (at
 *     l = 0 the caller's rim, untouched); for l >= 1 then `fmg` cycles as above started at level l from u_l on F_l (level l
 *     keeps its field, the levels below start from zero; the constants of every level, shift included, are the solve's).
 *     Level 0 gets no cycle inside the pass: the cycle loop follows.
 * A coarse solve of the pass that stops at its cap sets coarse_capped like one of a cycle.  The option needs
 * about N^2/3 more doubles of device memory (the F_l of the coarse levels; the g_l and the tables are O(N)), allocated at
 * creation when fmg >= 1.
 * mg_batch_solver_create refuses fmg != 0 with MG_ERR_ARG: the batched pass is not built yet.
 * ABI: `fmg` (version 0.2.1) sits in the alignment hole between max_cycles and shift: the size of the struct and the offset
 * of every 0.2 field are unchanged, shift stays the last field, and mg_solve_opts_default() of this library sets fmg = 0
 * in the struct of a caller compiled against the 0.2 header. */
typedef struct mg_solve_opts {
    int    pre, post;          /* sweeps per level on the way down / up, 1..4 */
    int    N_min;              /* coarsest size bound, 3..32 */
    double omega;              /* Jacobi weight, (0, 1] */
    double coarse_rtol, coarse_atol;
    int    coarse_max_iters;   /* >= 1; reaching it is reported (coarse_capped), not fatal */
    double rtol, atol;         /* stopping rule on the L2 residual */
    int    max_cycles;         /* >= 0 */
    int    fmg;                /* full-multigrid start: 0 = off, 1..8 = V-cycles per coarse level of the ascent */
    double shift;              /* sigma of Laplace(U) - sigma*U = F, finite and >= 0; 0: the Poisson equation (LAST field) */
} mg_solve_opts;

#define MG_SOLVE_CONVERGED      0
#define MG_SOLVE_NOT_CONVERGED (-1)   /* max_cycles cycles ran without meeting the tolerance */

typedef struct mg_solve_result {
    int    status;             /* MG_SOLVE_CONVERGED, MG_SOLVE_NOT_CONVERGED, or an error code (> 0, mg_last_error) */
    int    cycles;             /* V-cycles run */
    int    converged;
    int    coarse_capped;      /* 1 when some coarse solve stopped at coarse_max_iters above its target */
    double res0, res, ref_norm;   /* ||F - AU_0||, ||F - AU_cycles||, ||F|| (interior L2) */
    double device_ms;          /* hipEvent time of the whole call */
    int    n_history;          /* cycles + 1 */
    const double *history;     /* r_0 .. r_cycles, owned by the solver, valid until its next solve */
} mg_solve_result;

typedef struct mg_solver mg_solver;

/* V(3,3), omega 0.8, N_min 8, coarse_rtol 1e-2, coarse_atol 0, coarse_max_iters 10000, rtol 1e-10, atol 0, 50 cycles,
 * shift 0, fmg 0.
 * rtol is relative to ||F||: on large grids the fp64 rounding of inv*(star - 4U) (inv = 1/dx^2) puts a floor under the
 * reachable residual -- about 8e-10 relative at N = 8192 on the getSource problem -- so a default solve there runs all
 * max_cycles and returns MG_SOLVE_NOT_CONVERGED; ask for rtol >= 1e-9 at that size. */
void       mg_solve_opts_default(mg_solve_opts *o);
/* every level array is allocated here (NULL opts: the defaults); NULL on bad arguments (mg_last_error) */
mg_solver *mg_solver_create(int N, double L, const mg_solve_opts *o);
/* F_dev, U_dev: N x N device arrays (16-byte aligned).  Allocates nothing, works on the engine stream (mg_set_stream) and
 * reads one norm back per cycle.  Returns out->status.  The cycle runs through the fused nodes of the streaming smoother
 * (weighted instantiations); with mg_set_smoother("simple") operator by operator -- the same bits. */
int        mg_solver_solve(mg_solver *s, const double *F_dev, double *U_dev, mg_solve_result *out);
void       mg_solver_destroy(mg_solver *s);

/* ------------------------------------------------------------------------- */
/* batched residual-tolerance solver: B problems of one size and one set of   */
/* options in one call, each solved exactly as mg_solver_solve solves it      */
/* ------------------------------------------------------------------------- */
/* Instance i gives the same U, cycles, status, converged, coarse_capped, res0, res, ref_norm and history, bit for bit, as
 * mg_solver_solve on F_dev[i], U_dev[i] with the same options, whatever the other instances are and wherever it sits in
 * the batch.  An instance leaves the batch once it meets its own tolerance max(rtol*||F_i||, atol); its U is never written
 * after that (a start that meets it: 0 cycles, U untouched).  One cycle runs the single solve's launches ONCE over all
 * active instances (blockIdx picks the instance): the launches per cycle do not depend on the batch size.  Several
 * instances may share one F (the same source with different boundary values). */
typedef struct mg_batch_solve_stats {
    int    cycles;             /* the most cycles any instance ran */
    int    launches;           /* kernel launches the call enqueued */
    double device_ms;          /* hipEvent time of the whole call */
} mg_batch_solve_stats;

typedef struct mg_batch_solver mg_batch_solver;

/* every level array for max_batch instances, the per-instance norm partials and scalars and the pinned read-back buffers
 * are allocated here (NULL opts: the defaults; the options are checked as mg_solver_create checks them) */
mg_batch_solver *mg_batch_solver_create(int N, double L, int max_batch, const mg_solve_opts *o);
/* F_dev[i], U_dev[i]: host arrays of n device pointers to N x N arrays (each 16-byte aligned), 1 <= n <= max_batch; no two
 * U arrays overlap and no U overlaps an F (F pointers may repeat).  out: n results (out[i].device_ms: the whole call;
 * out[i].history: owned by the batch solver, valid until its next solve); stats may be NULL.  Allocates nothing, works on
 * the engine stream and reads the n norms back once per cycle in one copy.  Returns MG_SOLVE_CONVERGED when every
 * instance converged, MG_SOLVE_NOT_CONVERGED when at least one did not, an error code (> 0) otherwise (MG_ERR_ARG for bad
 * arguments, before anything is enqueued).  The cycle runs through batched launches of the fused nodes; with
 * mg_set_smoother("simple") operator by operator, instance by instance -- the same bits. */
int  mg_batch_solver_solve(mg_batch_solver *s, int n, const double *const *F_dev, double *const *U_dev, mg_solve_result *out,
                           mg_batch_solve_stats *stats);
void mg_batch_solver_destroy(mg_batch_solver *s);

#ifdef __cplusplus
}
#endif

/* the building blocks of the full-multigrid start (mg_solve_opts.fmg): mg_cubic_table, mg_prolongCubic */
#include "mg_fmg.h"
/* the recorded V-cycle both solvers walk, as a host-only list of its launches (for tests): mg_solve_cycle_describe */
#include "mg_solve_cycle.h"
/* time stepping of the heat equation over the solvers (theta-scheme): mg_heat_rhs, mg_heat_stepper_* */
#include "mg_heat.h"
/* the solver with a variable coefficient, div(a grad U) - sigma*U = F: mg_solver_set_coefficient, mg_applyOperator, ... */
#include "mg_varcoef.h"
/* the heat stepper with a variable coefficient, u_t = nu*div(a grad u) + q: mg_heat_rhs_coef, mg_heat_stepper_set_coefficient */
#include "mg_heat_vc.h"
/* the batched solver with a variable coefficient per instance (or one shared): mg_batch_solver_set_coefficient */
#include "mg_varcoef_batch.h"
/* adjoint sensitivities of a solve, gradients in F, the rim data and a(x, y): mg_solver_adjoint, mg_coefficientGradient, ... */
#include "mg_adjoint.h"
/* the lowest eigenmodes of -div(a grad u), multigrid-preconditioned LOBPCG: mg_eigs_create, mg_eigs_solve, ... */
#include "mg_eigs.h"
#include "mg_reaction.h"
/* the semilinear problem div(a grad U) - sigma*U - kappa*w*g(U) = F, Newton around the solver: mg_solver_newton, ... */
#include "mg_newton.h"
#include "mg_rx_batch.h"
#include "mg_newton_batch.h"
/* the adjoint of solves with s(x, y) and of semilinear solves, gradients in s, sigma, w and kappa: mg_sourceGradient, ... */
#include "mg_adjoint_rx.h"
/* Neumann and mixed boundary kinds per side in the solver and the heat stepper: mg_solver_set_boundary, mg_neumannSource, ... */
#include "mg_bc.h"
/* the batched solver with the Krylov acceleration, GCR(m) per instance: mg_batch_solver_set_krylov, ... */
#include "mg_krylov_batch.h"
/* Krylov acceleration of the residual-tolerance solver, restarted GCR(m) around the cycle: mg_solver_set_krylov, ... */
#include "mg_krylov.h"

#endif /* MG_HIP_H */
