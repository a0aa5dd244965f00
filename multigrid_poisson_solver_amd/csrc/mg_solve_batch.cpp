// mg_solve_batch.cpp -- batched residual-tolerance solver (include/mg_hip.h, "batched residual-tolerance solver"): n
// problems of one size and one set of options in one call, each instance bit-identical to mg_solver_solve alone.
// One cycle is the recorded SolveCycle that mg_solver walks (mg_internal.h, built by build_solve_cycle in mg_solve.cpp; DESIGN.md
// 4.3.8), for all active instances together: each of its steps becomes ONE launch over the active set, the instance taken
// from a NodeBatchItem table by blockIdx (the weighted streaming nodes, mg_stream_impl.h; the norm, coarse solve and transfer
// kernels, mg_solve_kernels.hip).  fill_slot writes an instance's arrays into the table of every step, run_cycle_batch issues
// the launches; neither knows the cycle's dataflow.
// After each read-back the host drops the instances that met their tolerance from the active set and rebuilds and
// uploads the tables when the set changed (the read-back already synchronises once per cycle, so one pinned staging
// buffer serves every upload).
// With a coefficient set (include/mg_varcoef_batch.h) the recorded cycle is the operator-by-operator one with the coefficient
// in its steps, through the batched `_vc` kernels (mg_varcoef_batch_kernels.hip).
// With mg_batch_solver_set_krylov(m > 0) (include/mg_krylov_batch.h) the loop is restarted GCR(m) per instance around either
// cycle: krylov_iterate_batch below, launch by launch over the active set (mg_krylov_batch_kernels.hip).
// With a reaction set (include/mg_rx_batch.h) the cycle is the operator-by-operator one too, with or without a coefficient,
// through the batched `_rx` kernels (mg_reaction_batch_kernels.hip): the level's reaction term rides in the slot `Fc` of the
// sweep, residual and coarse-solve tables, which the recorded steps leave empty -- the steps themselves do not change.
// mg_batch_solver_newton (include/mg_newton_batch.h) is Newton's method around that loop for all instances in lockstep: the
// batched pass of mg_newton_batch_kernels.hip, and solve_instances below on the instances that still iterate, whose level-0
// reaction term is whichever of the driver's two S sets holds the accepted iterate's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mg_internal.h"

using namespace mg;

struct mg_batch_solver {
    int N = 0;
    double L = 1.0;
    int max_batch = 0;
    mg_solve_opts o{};
    std::vector<int> sizes;                  // N, N/2, ... >= N_min
    std::vector<LevelConsts> lc;             // per level: spacing, centre coefficient, weight (mg_solver's)
    std::vector<size_t> pitch;               // doubles from one instance's level array to the next one's
    std::vector<double *> A, B, F;           // per level, max_batch instances each (level 0: only B)
    double *part = nullptr;                  // norm partials, resnorm_partials(N) per instance
    void *dev_rb = nullptr, *host_rb = nullptr;   // read-back block: res[max_batch], ref[max_batch], gs_state[4*max_batch]
    // the recorded cycles from level 0, set at creation: through the fused nodes, and operator by operator with the
    // coefficient in its steps (MG_SMOOTHER=simple walks the latter too: mg_solver's walk takes the coefficient from its
    // operator, which has none there)
    SolveCycle cyc_fused, cyc_ops;
    NodeBatchItem *dev_tab = nullptr, *host_tab = nullptr;   // [n_tables][max_batch]: table 0 the norm's, then the cycle's slots
    int n_tables = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_sync = nullptr;
    std::vector<std::vector<double>> history;   // per instance of the last solve
    // variable coefficient (include/mg_varcoef_batch.h; nothing of it is allocated before the first
    // mg_batch_solver_set_coefficient)
    std::vector<double *> coef;              // per level: the nodal coefficients of coef_cap instances at the instance pitch
    int coef_cap = 0;                        // instances the level storage holds
    int n_coef = 0;                          // 0: none set; 1: one shared by every instance; n > 1: instance i uses copy i
    int *coef_flags = nullptr;               // device [max_batch]: the check found a bad value in that instance
    int *host_coef_flags = nullptr;          // pinned [max_batch]
    // variable reaction term (include/mg_rx_batch.h; nothing of it is allocated before the first mg_batch_solver_set_reaction);
    // the check borrows coef_flags / host_coef_flags
    std::vector<double *> react;             // per level: the nodal reaction terms of react_cap instances at the instance pitch
    int react_cap = 0;                       // instances the level storage holds
    int n_react = 0;                         // 0: none set; 1: one shared by every instance; n > 1: instance i uses copy i
    // Krylov acceleration (include/mg_krylov_batch.h; nothing of it is allocated before the first enabling
    // mg_batch_solver_set_krylov).  Everything is indexed by the instance's position in the call, not by its active slot.
    int kr_m = 0;                            // 0: off
    double *kr_r = nullptr;                  // the residuals r_i, at the level-0 instance pitch
    std::vector<double *> kr_Z, kr_Q;        // the slots allocated so far: slot j holds z_j (q_j) of max_batch instances at that pitch
    double *kr_part = nullptr;               // partials: KRYLOV_MAX_K stripes of krylov_blocks(N) per instance
    double *kr_scal = nullptr;               // device [max_batch][KRYLOV_SCAL_COUNT]: b_j, w_j, alpha, breakdown
    double *kr_log = nullptr;                // device [max_batch][max(max_cycles, 1)] records of KR_REC_MAX doubles
    double *kr_rb = nullptr, *kr_host_rb = nullptr;   // read-back by active slot: rho_rec[max_batch], breakdown[max_batch] (pinned twin)
    void *kr_dev_tab = nullptr, *kr_host_tab = nullptr;   // one block, one upload: KrylovTables (below)
    std::vector<double> kr_log_host;         // the last solve's records, per instance max(max_cycles, 1) of kr_log_m + 7 doubles
    std::vector<int> kr_k, kr_records;       // per instance: its k, its records of the last solve
    std::vector<char> kr_brk;                // per instance: the last solve ended on a breakdown
    std::vector<const double *> kr_F;        // per instance: the cycle's F0 = r_i (MG_SMOOTHER=simple takes pointers by instance)
    std::vector<double *> kr_U;              // per instance: the cycle's U0 = z_k of this iteration
    int kr_log_m = 0, kr_n = 0;              // the m and the instances of the last accelerated solve
    // batched Newton driver (include/mg_newton_batch.h; nothing of it is allocated before the first mg_batch_solver_newton)
    double *nw_field = nullptr;              // 5 fields of max_batch instances each at the level-0 pitch: V, D, D', S', delta
    void *nw_dev = nullptr, *nw_host = nullptr;   // one block in device and one in pinned memory: NewtonBlock (below)
    hipEvent_t nw_ev_begin = nullptr, nw_ev_end = nullptr;
    std::vector<double *> nw_S0;             // per instance: its level-0 reaction term while nw_on (either of its two S sets)
    bool nw_on = false;                      // an inner solve of the driver is running: react_of takes level 0 from nw_S0
    std::vector<std::vector<mg_newton_iter>> nw_hist;   // per instance of the last call
    int nw_n = 0;                            // the instances of the last call
};

namespace {

size_t rb_bytes(int mb) { return (size_t)mb * (2 * sizeof(double) + 4 * sizeof(int)); }
double *rb_res(void *rb) { return static_cast<double *>(rb); }
double *rb_ref(void *rb, int mb) { return static_cast<double *>(rb) + mb; }
int *rb_state(void *rb, int mb) { return reinterpret_cast<int *>(static_cast<double *>(rb) + 2 * (size_t)mb); }

double *level(const mg_batch_solver *s, const std::vector<double *> &v, int l, int i) { return v[l] + (size_t)i * s->pitch[l]; }

void release(mg_batch_solver *s)
{
    for (double *p : s->A) if (p) (void)hipFree(p);
    for (double *p : s->B) if (p) (void)hipFree(p);
    for (double *p : s->F) if (p) (void)hipFree(p);
    for (double *p : s->coef) if (p) (void)hipFree(p);
    for (double *p : s->react) if (p) (void)hipFree(p);
    if (s->coef_flags) (void)hipFree(s->coef_flags);
    if (s->host_coef_flags) (void)hipHostFree(s->host_coef_flags);
    for (double *p : s->kr_Z) if (p) (void)hipFree(p);
    for (double *p : s->kr_Q) if (p) (void)hipFree(p);
    for (double *p : {s->kr_r, s->kr_part, s->kr_scal, s->kr_log, s->kr_rb}) if (p) (void)hipFree(p);
    if (s->kr_dev_tab) (void)hipFree(s->kr_dev_tab);
    if (s->kr_host_rb) (void)hipHostFree(s->kr_host_rb);
    if (s->kr_host_tab) (void)hipHostFree(s->kr_host_tab);
    if (s->nw_field) (void)hipFree(s->nw_field);
    if (s->nw_dev) (void)hipFree(s->nw_dev);
    if (s->nw_host) (void)hipHostFree(s->nw_host);
    if (s->nw_ev_begin) (void)hipEventDestroy(s->nw_ev_begin);
    if (s->nw_ev_end) (void)hipEventDestroy(s->nw_ev_end);
    if (s->part) (void)hipFree(s->part);
    if (s->dev_rb) (void)hipFree(s->dev_rb);
    if (s->host_rb) (void)hipHostFree(s->host_rb);
    if (s->dev_tab) (void)hipFree(s->dev_tab);
    if (s->host_tab) (void)hipHostFree(s->host_tab);
    if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
    if (s->ev_end) (void)hipEventDestroy(s->ev_end);
    if (s->ev_sync) (void)hipEventDestroy(s->ev_sync);
    delete s;
}

// the cycle the tables are built for: with a coefficient or a reaction operator by operator, whatever mg_set_smoother says
const SolveCycle &cycle_of(const mg_batch_solver *s) { return s->n_coef > 0 || s->n_react > 0 ? s->cyc_ops : s->cyc_fused; }

// the level-l reaction term of instance i (copy i, or the one copy in shared mode); nullptr without a reaction.  Inside
// mg_batch_solver_newton the level-0 term is the one of the driver's two S sets that holds the instance's accepted iterate's
double *react_of(const mg_batch_solver *s, int l, int i)
{
    if (l == 0 && s->nw_on) return s->nw_S0[i];
    return s->n_react > 0 ? level(s, s->react, l, s->n_react == 1 ? 0 : i) : nullptr;
}

// the arrays of instance i (active slot j) in the table of every step of the cycle; table 0: the norm's entry.  The coefficient
// is copy i, or the one copy in shared mode.  With a reaction the level's term goes into the slot `Fc` of the norm, the sweeps,
// the residuals and the coarse solve, whose steps record none there (and, without a coefficient, nothing into `coarse`)
void fill_slot(mg_batch_solver *s, const SolveCycle &c, int j, const double *F0, double *U0, int i)
{
    const int ci = s->n_coef == 1 ? 0 : i;
    auto at = [&](FieldRef r) -> double * {
        switch (r.f) {
        case Field::U0: return U0;
        case Field::F0: return const_cast<double *>(F0);
        case Field::A: return level(s, s->A, r.level, i);
        case Field::B: return level(s, s->B, r.level, i);
        case Field::F: return level(s, s->F, r.level, i);
        case Field::Coef: return s->n_coef > 0 ? level(s, s->coef, r.level, ci) : nullptr;
        case Field::None: break;
        }
        return nullptr;
    };
    auto item = [&](int t) -> NodeBatchItem & { return s->host_tab[(size_t)t * s->max_batch + j]; };
    item(0) = NodeBatchItem{U0, F0, s->n_coef > 0 ? level(s, s->coef, 0, ci) : nullptr, nullptr, react_of(s, 0, i)};
    for (const SolveStep &t : c.steps) {
        const bool op = t.kind == SolveStep::Sweep || t.kind == SolveStep::Residual || t.kind == SolveStep::Coarse;
        item(t.slot) = NodeBatchItem{at(t.in), at(t.F), at(t.coarse), at(t.out), op && s->n_react > 0 ? react_of(s, t.level, i) : at(t.Fc)};
    }
}

// (without a coefficient: no more tables, and bytes, than the solver uploaded before it knew of one)
bool upload_tables(mg_batch_solver *s, hipStream_t st)
{
    const size_t used = (size_t)cycle_of(s).n_slots + 1;
    return MG_HIP(hipMemcpyAsync(s->dev_tab, s->host_tab, used * s->max_batch * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st));
}

// one cycle of the n active instances whose tables are uploaded: every step ONE launch over them from the table of its slot,
// with the `_rx` kernels when a reaction is set, else the `_vc` kernels when a coefficient is; returns the launches it enqueued
int run_cycle_batch(mg_batch_solver *s, hipStream_t st, const SolveCycle &c, int n)
{
    const mg_solve_opts &o = s->o;
    const int nl = (int)s->sizes.size(), mb = s->max_batch;
    const bool vc = s->n_coef > 0, rx = s->n_react > 0;
    for (const SolveStep &t : c.steps) {
        const int l = t.level, N = s->sizes[l], M = l + 1 < nl ? s->sizes[l + 1] : 0;   // (M: the coarse size of a transfer)
        const LevelConsts &lc = s->lc[l];
        const NodeBatchItem *tab = s->dev_tab + (size_t)t.slot * mb;
        switch (t.kind) {
        case SolveStep::Node: {
            const NodeBatch nb{n, tab, nullptr};
            // (active slot 0 of the host table: the shape of the node)
            k::SmoothNode<double> nd = solve_cycle_node(t, s->sizes, s->lc, s->host_tab[(size_t)t.slot * mb]);
            nd.batch = &nb;
            k::jacobi_stream(st, nd);
            break;
        }
        case SolveStep::Sweep:
            if (rx) k::wjacobi_rx_batch(st, n, N, lc.dx2, lc.sd, o.omega, t.in.f == Field::None, vc, tab);
            else k::wjacobi_vc_batch(st, n, N, lc.dx2, lc.sd, o.omega, t.in.f == Field::None, tab);
            break;
        case SolveStep::Residual:
            if (rx) k::residual_rx_batch(st, n, N, lc.dx2, lc.inv, lc.sd, vc, tab, -1);
            else if (vc) k::residual_vc_batch(st, n, N, lc.inv, lc.sd, tab, -1);
            else k::residual_batch(st, n, N, lc.inv, tab, -1, lc.sh);
            break;
        case SolveStep::Restrict: k::restrict_batch(st, n, N, M, tab, restrict_table(N, M), +1); break;
        case SolveStep::Coarse:
            if (rx)
                k::gauss_seidel_relative_rx_batch(st, n, N, lc.dx2, lc.inv, lc.sd, vc, tab, o.coarse_atol, o.coarse_rtol, o.coarse_max_iters,
                                                  rb_state(s->dev_rb, mb));
            else if (vc)
                k::gauss_seidel_relative_vc_batch(st, n, N, lc.dx2, lc.inv, lc.sd, tab, o.coarse_atol, o.coarse_rtol, o.coarse_max_iters,
                                                  rb_state(s->dev_rb, mb));
            else
                k::gauss_seidel_relative_batch(st, n, N, lc.dx2, lc.inv, tab, o.coarse_atol, o.coarse_rtol, o.coarse_max_iters,
                                               rb_state(s->dev_rb, mb), lc.sh);
            break;
        case SolveStep::ProlongAdd: k::prolong_add_batch(st, n, M, N, tab, prolong_table(M, N)); break;
        case SolveStep::Copy: k::copy_batch(st, n, (size_t)N * N, tab); break;
        }
    }
    return (int)c.steps.size();
}

// the same cycle operator by operator, instance by instance (MG_SMOOTHER=simple): the yardstick of the batched launches
int vcycle_simple_each(mg_batch_solver *s, hipStream_t st, const std::vector<int> &act, const double *const *F0,
                       double *const *U0)
{
    const int nl = (int)s->sizes.size();
    int launches = 0;
    const SolveOperator op{&s->o, &s->sizes, &s->lc};   // (neither kinds nor a coefficient: the constant kernels)
    std::vector<double *> A(nl), B(nl), F(nl);          // the instance's level arrays
    for (size_t j = 0; j < act.size(); ++j) {
        const int i = act[j];
        for (int l = 0; l < nl; ++l) {
            A[l] = level(s, s->A, l, i);
            B[l] = level(s, s->B, l, i);
            F[l] = level(s, s->F, l, i);
        }
        const SolveLevels lv{&A, &B, &F, rb_state(s->dev_rb, s->max_batch) + 4 * j, nullptr};
        launches += run_solve_cycle(st, s->cyc_ops, lv, op, F0[i], U0[i]);
    }
    return launches;
}

int norms(mg_batch_solver *s, hipStream_t st, int n, bool has_u, double *out)
{
    k::resnorm_batch(st, n, s->N, s->lc[0].inv, has_u, s->dev_tab, s->part, out, s->lc[0].sh);
    return 2;
}

// the residual norm with the coefficient (the reference norm ||F|| has no operator in it: norms(..., false, ...))
int norms_vc(mg_batch_solver *s, hipStream_t st, int n, double *out)
{
    k::resnorm_vc_batch(st, n, s->N, s->lc[0].inv, s->lc[0].sd, s->dev_tab, s->part, out);
    return 2;
}

// the residual norm with the reaction (and the coefficient, when one is set)
int norms_rx(mg_batch_solver *s, hipStream_t st, int n, double *out)
{
    k::resnorm_rx_batch(st, n, s->N, s->lc[0].dx2, s->lc[0].inv, s->lc[0].sd, s->n_coef > 0, s->dev_tab, s->part, out);
    return 2;
}

// the stopping norm ||F - AU|| of the n instances of table 0 with the operator that is set
int norms_res(mg_batch_solver *s, hipStream_t st, int n, double *out)
{
    if (s->n_react > 0) return norms_rx(s, st, n, out);
    return s->n_coef > 0 ? norms_vc(s, st, n, out) : norms(s, st, n, true, out);
}

bool read_back(mg_batch_solver *s, hipStream_t st)
{
    if (!MG_HIP(hipMemcpyAsync(s->host_rb, s->dev_rb, rb_bytes(s->max_batch), hipMemcpyDeviceToHost, st))) return false;
    if (!MG_HIP(hipEventRecord(s->ev_sync, st))) return false;
    return MG_HIP(hipEventSynchronize(s->ev_sync));
}

bool overlap(const void *a, const void *b, size_t bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}


// ------------------------------------------------------------------ Krylov acceleration (include/mg_krylov_batch.h)
constexpr int KR_REC_MAX = MG_KRYLOV_MAX_M + 7;

// the tables of one iteration, one block in pinned and one in device memory, uploaded together: by active slot the Krylov
// kernels' entries and A*z (in = z_k, coarse = a_i or NULL, out = q_k, Fc = s_i or NULL); by slot of the restarting subset the
// record to mark and the residual and norm (in = U_i, F = F_i, coarse = a_i or NULL, out = r_i, Fc = s_i or NULL); `first` is
// the latter for the residual that starts the loop, a table of its own because it is uploaded while the first iteration's
// tables are written
struct KrylovTables {
    k::KrylovBatchItem *act, *mark;
    NodeBatchItem *apply, *recompute, *first;
};
size_t krylov_tables_bytes(int mb) { return (size_t)mb * (2 * sizeof(k::KrylovBatchItem) + 3 * sizeof(NodeBatchItem)); }
KrylovTables krylov_tables(void *base, int mb)
{
    KrylovTables t;
    t.act = static_cast<k::KrylovBatchItem *>(base);
    t.mark = t.act + mb;
    t.apply = reinterpret_cast<NodeBatchItem *>(t.mark + mb);
    t.recompute = t.apply + mb;
    t.first = t.recompute + mb;
    return t;
}
size_t krylov_log_stride(const mg_batch_solver *s) { return (size_t)(s->o.max_cycles > 0 ? s->o.max_cycles : 1) * KR_REC_MAX; }

// every table but `first` (which the call that starts the loop uploads alone)
bool krylov_upload(mg_batch_solver *s, hipStream_t st)
{
    const size_t bytes = krylov_tables_bytes(s->max_batch) - (size_t)s->max_batch * sizeof(NodeBatchItem);
    return MG_HIP(hipMemcpyAsync(s->kr_dev_tab, s->kr_host_tab, bytes, hipMemcpyHostToDevice, st));
}

// the read-back of an iteration: rho_rec and the breakdown flag of every active slot, and the block of read_back
bool krylov_read_back(mg_batch_solver *s, hipStream_t st)
{
    if (!MG_HIP(hipMemcpyAsync(s->kr_host_rb, s->kr_rb, 2 * (size_t)s->max_batch * sizeof(double), hipMemcpyDeviceToHost, st))) return false;
    return read_back(s, st);
}

// The loop of include/mg_krylov.h for every instance of `act` (those above their tolerance after history[0]), each with its
// own k, tolerance and restart decisions; one launch per kernel of the single solver's iteration over the active set
// (include/mg_krylov_batch.h).  members: the instances the solve started with, whose state is reset.  false on a HIP error.
bool krylov_iterate_batch(mg_batch_solver *s, hipStream_t st, int n, const double *const *F_dev, double *const *U_dev,
                          const std::vector<double> &tol, std::vector<mg_solve_result> &r, mg_batch_solve_stats &bs,
                          const std::vector<int> &members, std::vector<int> act)
{
    const mg_solve_opts &o = s->o;
    const int N = s->N, m = s->kr_m, rec_len = m + 7, mb = s->max_batch;
    const size_t p0 = s->pitch[0], n_part = (size_t)k::KRYLOV_MAX_K * k::krylov_blocks(N), log_stride = krylov_log_stride(s);
    const double pts = (double)N * N, sd = s->lc[0].sd;
    const bool vc = s->n_coef > 0, rx = s->n_react > 0, simple = ctx().smoother == SMOOTHER_SIMPLE;
    const double dx2 = s->lc[0].dx2;
    const KrylovTables host = krylov_tables(s->kr_host_tab, mb), dev = krylov_tables(s->kr_dev_tab, mb);
    s->kr_log_m = m;
    s->kr_n = n;
    for (int i : members) {   // (the instances of this solve: 0 .. n-1, or those of a Newton call that still iterate)
        s->kr_k[i] = s->kr_records[i] = 0;
        s->kr_brk[i] = 0;
    }
    k::KrylovVecs v{};
    for (int j = 0; j < m && j < k::KRYLOV_MAX_K; ++j) {
        v.q[j] = s->kr_Q[j];
        v.z[j] = s->kr_Z[j];
    }
    auto coef_of = [&](int i) -> const double * { return vc ? level(s, s->coef, 0, s->n_coef == 1 ? 0 : i) : nullptr; };
    auto rec_of = [&](int i) { return s->kr_log + (size_t)i * log_stride + (size_t)r[i].cycles * rec_len; };
    // r = -(inv*b(U) - F) and ||F - AU|| of the instances `sub`, whose table entries are uploaded: the launches of the
    // batched cycle's signed residual at level 0 and of the stopping norm, into rb_res by slot of `sub`
    auto fill_recompute = [&](const std::vector<int> &sub) {
        for (size_t js = 0; js < sub.size(); ++js) {
            const int i = sub[js];
            host.recompute[js] = NodeBatchItem{U_dev[i], F_dev[i], coef_of(i), s->kr_r + (size_t)i * p0, react_of(s, 0, i)};
            host.mark[js] = k::KrylovBatchItem{};
            host.mark[js].rec = rec_of(i);
        }
    };
    auto residual = [&](int ns, const NodeBatchItem *items) {
        ProfScope ps("krylov_residual_batch", N, pts * ns * ((vc ? 32.0 : 24.0) + (rx ? 8.0 : 0.0)));
        if (rx) k::residual_rx_batch(st, ns, N, dx2, s->lc[0].inv, sd, vc, items, -1);
        else if (vc) k::residual_vc_batch(st, ns, N, s->lc[0].inv, sd, items, -1);
        else k::residual_batch(st, ns, N, s->lc[0].inv, items, -1, s->lc[0].sh);
        return 1;
    };
    auto recompute = [&](int ns) {
        int launches = residual(ns, dev.recompute);
        if (rx) k::resnorm_rx_batch(st, ns, N, dx2, s->lc[0].inv, sd, vc, dev.recompute, s->part, rb_res(s->dev_rb));
        else if (vc) k::resnorm_vc_batch(st, ns, N, s->lc[0].inv, sd, dev.recompute, s->part, rb_res(s->dev_rb));
        else k::resnorm_batch(st, ns, N, s->lc[0].inv, true, dev.recompute, s->part, rb_res(s->dev_rb), s->lc[0].sh);
        k::krylov_log_restart_batch(st, ns, m, dev.mark, rb_res(s->dev_rb));
        return launches + 3;
    };
    if (act.empty()) return true;
    for (size_t j = 0; j < act.size(); ++j)
        host.first[j] = NodeBatchItem{U_dev[act[j]], F_dev[act[j]], coef_of(act[j]), s->kr_r + (size_t)act[j] * p0, react_of(s, 0, act[j])};
    if (!MG_HIP(hipMemcpyAsync(dev.first, host.first, act.size() * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st))) return false;
    bs.launches += residual((int)act.size(), dev.first);
    std::vector<int> known, late, next;   // restarts known before the read-back (k + 1 == m), and found by it
    std::vector<double> res(n, 0.0);
    while (!act.empty()) {
        const int na = (int)act.size();
        int kmax = 0;
        double dots_bytes = 0.0, orth_bytes = 0.0;
        known.clear();
        for (int j = 0; j < na; ++j) {
            const int i = act[j], kk = s->kr_k[i];
            double *ri = s->kr_r + (size_t)i * p0, *z = s->kr_Z[kk] + (size_t)i * p0, *q = s->kr_Q[kk] + (size_t)i * p0;
            s->kr_F[i] = ri;
            s->kr_U[i] = z;
            fill_slot(s, cycle_of(s), j, ri, z, i);
            host.act[j] = k::KrylovBatchItem{U_dev[i], ri, z, q, s->kr_scal + (size_t)i * k::KRYLOV_SCAL_COUNT,
                                             s->kr_part + (size_t)i * n_part, rec_of(i), (size_t)i * p0, kk, 0};
            host.apply[j] = NodeBatchItem{z, nullptr, coef_of(i), q, react_of(s, 0, i)};
            if (kk > kmax) kmax = kk;
            dots_bytes += kk > 0 ? 8.0 + 8.0 * kk : 0.0;
            orth_bytes += kk > 0 ? 40.0 + 16.0 * kk : 16.0;
            if (kk + 1 == m) known.push_back(i);
        }
        fill_recompute(known);
        if (!upload_tables(s, st) || !krylov_upload(s, st)) return false;
        {
            ProfScope ps("krylov_zero_batch", N, pts * na * 8.0);
            k::krylov_zero_batch(st, na, N, dev.act);
        }
        bs.launches += 1;
        bs.launches += simple && !vc && !rx ? vcycle_simple_each(s, st, act, s->kr_F.data(), s->kr_U.data())
                                     : run_cycle_batch(s, st, cycle_of(s), na);
        {
            ProfScope ps("krylov_apply_batch", N, pts * na * ((vc ? 24.0 : 16.0) + (rx ? 8.0 : 0.0)));
            if (rx) k::apply_rx_batch(st, na, N, dx2, s->lc[0].inv, sd, vc, dev.apply);
            else k::apply_vc_batch(st, na, N, s->lc[0].inv, sd, dev.apply);
        }
        bs.launches += 1;
        if (kmax > 0) {
            ProfScope ps("krylov_dots_batch", N, pts * dots_bytes);
            k::krylov_dots_batch(st, na, N, kmax, dev.act, v);
            bs.launches += 2;
        }
        {
            ProfScope ps("krylov_orth_batch", N, pts * orth_bytes);
            k::krylov_orth_batch(st, na, N, kmax, m, dev.act, v);
        }
        {
            ProfScope ps("krylov_update_batch", N, pts * na * 48.0);
            k::krylov_update_batch(st, na, N, m, dev.act, s->kr_rb, mb);
        }
        bs.launches += 4;
        if (!known.empty()) bs.launches += recompute((int)known.size());
        if (!krylov_read_back(s, st)) return false;
        late.clear();
        size_t at_known = 0;
        for (int j = 0; j < na; ++j) {
            const int i = act[j];
            if (at_known < known.size() && known[at_known] == i) {
                res[i] = rb_res(s->host_rb)[at_known++];
            } else {
                res[i] = s->kr_host_rb[j];
                if (res[i] <= tol[i]) late.push_back(i);
            }
            if (rb_state(s->host_rb, mb)[4 * j + 2]) r[i].coarse_capped = 1;
            if (s->kr_host_rb[mb + j] != 0.0) s->kr_brk[i] = 1;
        }
        if (!late.empty()) {   // the recurred norm met the tolerance: the recomputed one decides
            fill_recompute(late);
            if (!krylov_upload(s, st)) return false;
            bs.launches += recompute((int)late.size());
            if (!read_back(s, st)) return false;
            for (size_t js = 0; js < late.size(); ++js) res[late[js]] = rb_res(s->host_rb)[js];
        }
        for (int i : known) s->kr_k[i] = -1;
        for (int i : late) s->kr_k[i] = -1;
        next.clear();
        for (int j = 0; j < na; ++j) {
            const int i = act[j];
            r[i].cycles += 1;
            s->kr_k[i] += 1;   // (0 after a restart)
            s->kr_records[i] = r[i].cycles;
            r[i].res = res[i];
            s->history[i].push_back(res[i]);
            if (r[i].cycles > bs.cycles) bs.cycles = r[i].cycles;
            if (!s->kr_brk[i] && !(res[i] <= tol[i]) && r[i].cycles < o.max_cycles) next.push_back(i);
        }
        act.swap(next);
    }
    return MG_HIP(hipMemcpyAsync(s->kr_log_host.data(), s->kr_log, (size_t)n * log_stride * sizeof(double), hipMemcpyDeviceToHost, st));
}

// the F and U of the n instances of a call: none NULL or misaligned, no U overlapping another U or any F
bool instances_ok(const char *who, const mg_batch_solver *s, int n, const double *const *F_dev, double *const *U_dev)
{
    const size_t bytes = (size_t)s->N * s->N * sizeof(double);
    for (int i = 0; i < n; ++i) {
        if (!F_dev[i] || !U_dev[i]) {
            fail(MG_ERR_ARG, "%s: NULL F or U of instance %d", who, i);
            return false;
        }
        if (((uintptr_t)F_dev[i] | (uintptr_t)U_dev[i]) % 16 != 0) {
            fail(MG_ERR_ARG, "%s: F and U of instance %d must be 16-byte aligned", who, i);
            return false;
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (j > i && overlap(U_dev[i], U_dev[j], bytes)) {
                fail(MG_ERR_ARG, "%s: U of instances %d and %d overlap", who, i, j);
                return false;
            }
            if (overlap(U_dev[i], F_dev[j], bytes)) {
                fail(MG_ERR_ARG, "%s: U of instance %d overlaps F of instance %d", who, i, j);
                return false;
            }
        }
    return true;
}

// mg_batch_solver_solve's loop on the instances `start` of a call of n (ascending positions: 0 .. n-1 for mg_batch_solver_solve
// itself; for mg_batch_solver_newton those that still iterate).  F_dev, U_dev, r, the level storage, the reaction copies and the
// Krylov state are indexed by the position in the call, tables and read-backs by active slot; r[i] and history[i] of the
// instances of `start` arrive zeroed.  Returns MG_SOLVE_CONVERGED, MG_SOLVE_NOT_CONVERGED (over `start`) or MG_ERR_HIP.
int solve_instances(mg_batch_solver *s, int n, const double *const *F_dev, double *const *U_dev, const std::vector<int> &start,
                    std::vector<mg_solve_result> &r, mg_batch_solve_stats &bs)
{
    const hipStream_t st = ctx().stream;
    const mg_solve_opts &o = s->o;
    const int mb = s->max_batch;
    const bool ops = s->n_coef > 0 || s->n_react > 0;   // (the operator-by-operator cycle, whatever mg_set_smoother says)
    const bool simple = ctx().smoother == SMOOTHER_SIMPLE;
    std::vector<int> act(start);
    std::vector<double> tol(n);
    const int n0 = (int)start.size();
    auto build = [&]() {
        for (size_t j = 0; j < act.size(); ++j)
            fill_slot(s, cycle_of(s), (int)j, F_dev[act[j]], U_dev[act[j]], act[j]);
        return upload_tables(s, st);
    };
    if (!MG_HIP(hipEventRecord(s->ev_begin, st))) return MG_ERR_HIP;
    if (!build()) return MG_ERR_HIP;
    bs.launches += norms(s, st, n0, false, rb_ref(s->dev_rb, mb));
    bs.launches += norms_res(s, st, n0, rb_res(s->dev_rb));
    if (!read_back(s, st)) return MG_ERR_HIP;
    std::vector<int> next;
    for (int j = 0; j < n0; ++j) {
        const int i = start[j];
        r[i].ref_norm = rb_ref(s->host_rb, mb)[j];
        r[i].res0 = r[i].res = rb_res(s->host_rb)[j];
        s->history[i].push_back(r[i].res);
        tol[i] = std::fmax(o.rtol * r[i].ref_norm, o.atol);
        if (!(r[i].res <= tol[i]) && o.max_cycles > 0) next.push_back(i);
    }
    if (s->kr_m > 0) {   // (the plain loop below then has nothing to do)
        if (!krylov_iterate_batch(s, st, n, F_dev, U_dev, tol, r, bs, start, next)) return MG_ERR_HIP;
        next.clear();
    }
    while (!next.empty()) {
        if (next != act) {   // the active set changed: compact it, rebuild and upload the tables
            act.swap(next);
            if (!build()) return MG_ERR_HIP;
        }
        const int na = (int)act.size();
        bs.launches += simple && !ops ? vcycle_simple_each(s, st, act, F_dev, U_dev) : run_cycle_batch(s, st, cycle_of(s), na);
        bs.launches += norms_res(s, st, na, rb_res(s->dev_rb));
        if (!read_back(s, st)) return MG_ERR_HIP;
        next.clear();
        for (int j = 0; j < na; ++j) {
            const int i = act[j];
            r[i].res = rb_res(s->host_rb)[j];
            s->history[i].push_back(r[i].res);
            r[i].cycles += 1;
            if (rb_state(s->host_rb, mb)[4 * j + 2]) r[i].coarse_capped = 1;
            if (r[i].cycles > bs.cycles) bs.cycles = r[i].cycles;
            if (!(r[i].res <= tol[i]) && r[i].cycles < o.max_cycles) next.push_back(i);
        }
    }
    if (!MG_HIP(hipEventRecord(s->ev_end, st)) || !MG_HIP(hipEventSynchronize(s->ev_end))) return MG_ERR_HIP;
    float ms = 0.0f;
    if (MG_HIP(hipEventElapsedTime(&ms, s->ev_begin, s->ev_end))) bs.device_ms = ms;
    bool all = true;
    for (int i : start) {
        r[i].converged = r[i].res <= tol[i] ? 1 : 0;
        r[i].status = r[i].converged ? MG_SOLVE_CONVERGED : MG_SOLVE_NOT_CONVERGED;
        all = all && r[i].converged;
    }
    return all ? MG_SOLVE_CONVERGED : MG_SOLVE_NOT_CONVERGED;
}

// ------------------------------------------------------------------ batched Newton driver (include/mg_newton_batch.h)
// the driver's tables and norms, one block in pinned and one in device memory: per level below the finest the coarsening of S
// (in = level l, out = level l + 1) by slot of the iterating instances, which also serves the copy home; the pass's items by slot
// of its launch; the norms of that launch by slot.  The solver's own tables are not borrowed: a solve rewrites them on the host
// while an upload enqueued here could still be reading them.
struct NewtonBlock {
    NodeBatchItem *coarsen;   // [max(nl - 1, 1)][mb]
    k::NewtonBatchItem *pass;
    double *norms;
};
size_t newton_block_bytes(int nl, int mb)
{
    return (size_t)mb * ((size_t)std::max(nl - 1, 1) * sizeof(NodeBatchItem) + sizeof(k::NewtonBatchItem) + sizeof(double));
}
NewtonBlock newton_block(void *base, int nl, int mb)
{
    NewtonBlock b;
    b.coarsen = static_cast<NodeBatchItem *>(base);
    b.pass = reinterpret_cast<k::NewtonBatchItem *>(b.coarsen + (size_t)std::max(nl - 1, 1) * mb);
    b.norms = reinterpret_cast<double *>(b.pass + mb);
    return b;
}

// what the first mg_batch_solver_newton allocates, all for max_batch instances (the byte count: include/mg_newton_batch.h);
// later calls find everything there.  The reaction's level storage is replaced only when it holds fewer instances than
// max_batch -- no reaction is set here, so nothing of value is in it.  false on a HIP error (the next call starts over).
bool newton_storage(mg_batch_solver *s)
{
    const int nl = (int)s->sizes.size(), mb = s->max_batch;
    const hipStream_t st = ctx().stream;
    bool poisoned = false;
    if (!s->coef_flags &&
        !(MG_HIP(hipMalloc((void **)&s->coef_flags, mb * sizeof(int))) &&
          MG_HIP(hipHostMalloc((void **)&s->host_coef_flags, mb * sizeof(int), hipHostMallocDefault)))) {
        if (s->coef_flags) { (void)hipFree(s->coef_flags); s->coef_flags = nullptr; }
        return false;
    }
    if (s->react_cap < mb) {
        std::vector<double *> fresh(nl, nullptr);
        for (int l = 0; l < nl; ++l)
            if (!MG_HIP(hipMalloc((void **)&fresh[l], s->pitch[l] * mb * sizeof(double)))) {
                for (double *p : fresh) if (p) (void)hipFree(p);
                return false;
            }
        if (!MG_HIP(hipStreamSynchronize(st))) {   // (nothing enqueued still reads the old set)
            for (double *p : fresh) (void)hipFree(p);
            return false;
        }
        for (double *p : s->react) if (p) (void)hipFree(p);
        s->react.swap(fresh);
        s->react_cap = mb;
        if (pool_poison_wanted()) {
            for (int l = 0; l < nl; ++l) poison_block(s->react[l], s->pitch[l] * mb * sizeof(double));
            poisoned = true;
        }
    }
    if (!s->nw_field) {
        const size_t field_bytes = 5 * s->pitch[0] * mb * sizeof(double), block = newton_block_bytes(nl, mb);
        double *field = nullptr;
        void *dev = nullptr, *host = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (!(MG_HIP(hipMalloc((void **)&field, field_bytes)) && MG_HIP(hipMalloc(&dev, block)) &&
              MG_HIP(hipHostMalloc(&host, block, hipHostMallocDefault)) && MG_HIP(hipEventCreate(&e0)) && MG_HIP(hipEventCreate(&e1)))) {
            if (field) (void)hipFree(field);
            if (dev) (void)hipFree(dev);
            if (host) (void)hipHostFree(host);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            return false;
        }
        std::memset(host, 0, block);
        s->nw_field = field;
        s->nw_dev = dev;
        s->nw_host = host;
        s->nw_ev_begin = e0;
        s->nw_ev_end = e1;
        s->nw_S0.assign(mb, nullptr);
        s->nw_hist.resize(mb);
        if (pool_poison_wanted()) {
            poison_block(field, field_bytes);
            poisoned = true;
        }
    }
    return !poisoned || MG_HIP(hipStreamSynchronize(st));
}

bool newton_kind_ok(const char *who, int kind)
{
    if (kind == MG_NEWTON_CUBIC || kind == MG_NEWTON_SINH || kind == MG_NEWTON_EXP) return true;
    fail(MG_ERR_ARG, "%s: unknown kind %d (MG_NEWTON_CUBIC = 0, MG_NEWTON_SINH = 1, MG_NEWTON_EXP = 2)", who, kind);
    return false;
}

// a count of optional per-instance arrays (0 / 1 shared / n) and its entries
bool optional_arrays_ok(const char *who, const char *what, int n, int count, const double *const *arr)
{
    if (count != 0 && count != 1 && count != n) {
        fail(MG_ERR_ARG, "%s: %d %s arrays for %d instances (0: none, 1: one shared by all, or one per instance)", who, count, what, n);
        return false;
    }
    if ((count == 0) != (arr == nullptr)) {
        fail(MG_ERR_ARG, "%s: %d %s arrays need %s", who, count, what, count == 0 ? "a NULL array" : "an array of device pointers");
        return false;
    }
    for (int i = 0; i < count; ++i)
        if (!arr[i] || (uintptr_t)arr[i] % 16 != 0) {
            fail(MG_ERR_ARG, "%s: the %s of instance %d is NULL or not 16-byte aligned", who, what, i);
            return false;
        }
    return true;
}

bool kappas_ok(const char *who, int n, const double *kappa)
{
    for (int i = 0; i < n; ++i)
        if (!(kappa[i] >= 0.0) || !std::isfinite(kappa[i])) {
            fail(MG_ERR_ARG, "%s: kappa = %g of instance %d must be finite and >= 0", who, kappa[i], i);
            return false;
        }
    return true;
}

}  // namespace

int mg::batch_solver_size(const mg_batch_solver *s, double *L, int *max_batch)
{
    if (L) *L = s->L;
    if (max_batch) *max_batch = s->max_batch;
    return s->N;
}

const double *mg::batch_solver_coefficient(const mg_batch_solver *s, int i)
{
    if (!s || s->n_coef == 0 || i < 0) return nullptr;
    if (s->n_coef == 1) return s->coef[0];
    return i < s->n_coef ? s->coef[0] + (size_t)i * s->pitch[0] : nullptr;
}

int mg::batch_solver_cycle(mg_batch_solver *s, hipStream_t st, int n, const double *const *F0, double *const *U0)
{
    std::vector<int> act(n);
    for (int i = 0; i < n; ++i) {
        act[i] = i;
        fill_slot(s, cycle_of(s), i, F0[i], U0[i], i);
    }
    if (!upload_tables(s, st)) return -1;
    if (s->n_coef == 0 && s->n_react == 0 && ctx().smoother == SMOOTHER_SIMPLE) return vcycle_simple_each(s, st, act, F0, U0);
    return run_cycle_batch(s, st, cycle_of(s), n);
}

bool mg::batch_solver_enqueue_state(mg_batch_solver *s, hipStream_t st)
{
    return MG_HIP(hipMemcpyAsync(s->host_rb, s->dev_rb, rb_bytes(s->max_batch), hipMemcpyDeviceToHost, st));
}

bool mg::batch_solver_coarse_capped(const mg_batch_solver *s, int n)
{
    for (int j = 0; j < n; ++j)
        if (rb_state(s->host_rb, s->max_batch)[4 * j + 2]) return true;
    return false;
}

// mg_batch_solver_newton's refusals, check of w and first pass over all n instances -- S straight into the level-0 reaction
// storage of each, D into the driver's field 1 and dropped -- then one coarsening launch per level; no lockstep is needed
int mg::batch_solver_newton_linearise(mg_batch_solver *s, const char *who, int n, int kind, const double *kappa, int n_w,
                                      const double *const *w_dev, const double *const *F_dev, const double *const *U_dev, double *norms,
                                      int *launches)
{
    if (s->n_react > 0) {
        fail(MG_ERR_UNSUPPORTED, "%s: a reaction term is set; the driver installs the Newton matrices' own (take yours away with "
                                 "mg_batch_solver_set_reaction(s, 0, NULL), or put it into w)", who);
        return MG_ERR_UNSUPPORTED;
    }
    if (n < 1 || n > s->max_batch) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, max_batch = %d]", who, n, s->max_batch);
        return MG_ERR_ARG;
    }
    if (s->n_coef > 1 && n > s->n_coef) {
        fail(MG_ERR_ARG, "%s: n = %d instances, but the solver holds %d coefficients (one per instance)", who, n, s->n_coef);
        return MG_ERR_ARG;
    }
    if (!optional_arrays_ok(who, "w", n, n_w, w_dev) || !newton_kind_ok(who, kind) || !kappas_ok(who, n, kappa)) return MG_ERR_ARG;
    const hipStream_t st = ctx().stream;
    const int N = s->N, nl = (int)s->sizes.size(), mb = s->max_batch;
    const size_t n0 = (size_t)N * N, p0 = s->pitch[0];
    const bool has_a = s->n_coef > 0, has_w = n_w > 0;
    if (!newton_storage(s)) return MG_ERR_HIP;
    if (has_w) {
        for (int i = 0; i < n_w; ++i) s->host_tab[i] = NodeBatchItem{w_dev[i], nullptr, nullptr, nullptr, nullptr};
        if (!MG_HIP(hipMemcpyAsync(s->dev_tab, s->host_tab, (size_t)n_w * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)) ||
            !MG_HIP(hipMemsetAsync(s->coef_flags, 0, n_w * sizeof(int), st)))
            return MG_ERR_HIP;
        k::reaction_check_batch(st, n_w, n0, s->dev_tab, s->coef_flags);
        *launches += 1;
        if (!MG_HIP(hipMemcpyAsync(s->host_coef_flags, s->coef_flags, n_w * sizeof(int), hipMemcpyDeviceToHost, st)) ||
            !MG_HIP(hipStreamSynchronize(st)))
            return MG_ERR_HIP;
        for (int i = 0; i < n_w; ++i)
            if (s->host_coef_flags[i]) {
                fail(MG_ERR_ARG, "%s: every value of w must be finite and >= 0 (instance %d has one that is not)", who, i);
                return MG_ERR_ARG;
            }
    }
    const LevelConsts &c0 = s->lc[0];
    const NewtonBlock host = newton_block(s->nw_host, nl, mb), dev = newton_block(s->nw_dev, nl, mb);
    for (int i = 0; i < n; ++i) {
        host.pass[i] = k::NewtonBatchItem{has_a ? level(s, s->coef, 0, s->n_coef == 1 ? 0 : i) : nullptr, has_w ? w_dev[n_w == 1 ? 0 : i] : nullptr,
                                          U_dev[i], nullptr, F_dev[i], nullptr, s->nw_field + (1 * (size_t)mb + i) * p0,
                                          level(s, s->react, 0, i), kappa[i]};
        for (int l = 0; l + 1 < nl; ++l)
            host.coarsen[(size_t)l * mb + i] = NodeBatchItem{level(s, s->react, l, i), nullptr, nullptr, level(s, s->react, l + 1, i), nullptr};
    }
    if (!MG_HIP(hipMemcpyAsync(dev.pass, host.pass, (size_t)n * sizeof(k::NewtonBatchItem), hipMemcpyHostToDevice, st))) return MG_ERR_HIP;
    k::newton_residual_batch(st, n, N, c0.inv, c0.sd, kind, has_a, has_w, false, 0.0, dev.pass, s->part, dev.norms);
    *launches += 2;
    if (!MG_HIP(hipMemcpyAsync(host.norms, dev.norms, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st)) ||
        !MG_HIP(hipEventRecord(s->ev_sync, st)) || !MG_HIP(hipEventSynchronize(s->ev_sync)))
        return MG_ERR_HIP;
    for (int i = 0; i < n; ++i) {
        if (norms) norms[i] = host.norms[i];
        if (!std::isfinite(host.norms[i])) {
            fail(MG_ERR_ARG, "%s: the residual of U of instance %d is not finite (%g)", who, i, host.norms[i]);
            return MG_ERR_ARG;
        }
    }
    if (nl > 1 && !MG_HIP(hipMemcpyAsync(dev.coarsen, host.coarsen, (size_t)(nl - 1) * mb * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)))
        return MG_ERR_HIP;
    for (int l = 0; l + 1 < nl; ++l)
        k::coef_coarsen_batch(st, n, s->sizes[l], s->sizes[l + 1], dev.coarsen + (size_t)l * mb, restrict_table(s->sizes[l], s->sizes[l + 1]));
    *launches += nl - 1;
    s->n_react = n;
    return MG_OK;
}

void mg::batch_solver_drop_reaction(mg_batch_solver *s)
{
    if (s) s->n_react = 0;
}

extern "C" {

mg_batch_solver *mg_batch_solver_create(int N, double L, int max_batch, const mg_solve_opts *opts)
{
    if (!require_ready("mg_batch_solver_create")) return nullptr;
    mg_solve_opts o;
    mg_solve_opts_default(&o);
    if (opts) o = *opts;
    if (!solve_opts_ok("mg_batch_solver_create", N, L, o)) return nullptr;
    if (o.fmg != 0) {   // (the batched full-multigrid pass is not built: refused, never ignored)
        fail(MG_ERR_ARG, "mg_batch_solver_create: fmg = %d is not supported by the batched solver (use mg_solver_create)", o.fmg);
        return nullptr;
    }
    if (max_batch < 1 || max_batch > 65535) {
        fail(MG_ERR_ARG, "mg_batch_solver_create: max_batch = %d outside [1, 65535]", max_batch);
        return nullptr;
    }
    mg_batch_solver *s = new mg_batch_solver;
    s->N = N;
    s->L = L;
    s->max_batch = max_batch;
    s->o = o;
    for (int n = N; n >= o.N_min; n /= 2) s->sizes.push_back(n);   // mg_solver_create's hierarchy
    const int nl = (int)s->sizes.size();
    s->lc = solve_level_consts(s->sizes, L, o);
    if (!k::gs_relative_fits(s->sizes[nl - 1])) {
        fail(MG_ERR_UNSUPPORTED, "mg_batch_solver_create: coarsest level %d does not fit the coarse solver", s->sizes[nl - 1]);
        release(s);
        return nullptr;
    }
    s->A.assign(nl, nullptr);
    s->B.assign(nl, nullptr);
    s->F.assign(nl, nullptr);
    s->pitch.assign(nl, 0);
    bool ok = true;
    for (int l = 0; l < nl && ok; ++l) {
        // (instance pitch rounded up to 256 B: every instance's rows start where a lone allocation's would)
        s->pitch[l] = ((size_t)s->sizes[l] * s->sizes[l] + 31) / 32 * 32;
        const size_t bytes = s->pitch[l] * max_batch * sizeof(double);
        ok = MG_HIP(hipMalloc((void **)&s->B[l], bytes));
        if (ok && l > 0) ok = MG_HIP(hipMalloc((void **)&s->A[l], bytes)) && MG_HIP(hipMalloc((void **)&s->F[l], bytes));
        if (ok && pool_poison_wanted())   // MG_POOL_POISON: no level array starts from what hipMalloc happened to return
            for (double *a : {s->A[l], s->B[l], s->F[l]}) poison_block(a, bytes);
    }
    for (int l = 0; l + 1 < nl && ok; ++l) {
        const int Nf = s->sizes[l], Nc = s->sizes[l + 1];
        ok = restrict_table(Nf, Nc).lo != nullptr && prolong_table(Nc, Nf).owner_row != nullptr;
    }
    if (ok) {
        std::vector<int> down_fused, up_fused;
        solve_fusable_levels(s->sizes, &down_fused, &up_fused);
        s->cyc_fused = build_solve_cycle(nl, o.pre, o.post, 0, true, down_fused.data(), up_fused.data(), false);
        s->cyc_ops = build_solve_cycle(nl, o.pre, o.post, 0, false, nullptr, nullptr, true);
    }
    // the norm's table and the slots of the larger cycle (a coefficient may be set later, and a solve allocates nothing); at
    // least nl tables, which mg_batch_solver_set_coefficient borrows for its check and coarsening launches
    s->n_tables = std::max(nl, std::max(s->cyc_fused.n_slots, s->cyc_ops.n_slots) + 1);
    const size_t tab_bytes = (size_t)s->n_tables * max_batch * sizeof(NodeBatchItem);
    ok = ok && MG_HIP(hipMalloc((void **)&s->part, k::resnorm_partials(N) * max_batch * sizeof(double))) &&
         MG_HIP(hipMalloc(&s->dev_rb, rb_bytes(max_batch))) &&
         MG_HIP(hipHostMalloc(&s->host_rb, rb_bytes(max_batch), hipHostMallocDefault)) &&
         MG_HIP(hipMalloc((void **)&s->dev_tab, tab_bytes)) &&
         MG_HIP(hipHostMalloc((void **)&s->host_tab, tab_bytes, hipHostMallocDefault)) &&
         MG_HIP(hipEventCreate(&s->ev_begin)) && MG_HIP(hipEventCreate(&s->ev_end)) &&
         MG_HIP(hipEventCreateWithFlags(&s->ev_sync, hipEventDisableTiming));
    if (ok && pool_poison_wanted()) poison_block(s->part, k::resnorm_partials(N) * max_batch * sizeof(double));
    ok = ok && MG_HIP(hipStreamSynchronize(ctx().stream));   // (the fills ran on the engine's stream; a solve may run on another)
    ok = ok && MG_HIP(hipMemset(s->dev_rb, 0, rb_bytes(max_batch)));
    if (!ok) {
        release(s);
        return nullptr;
    }
    std::memset(s->host_tab, 0, tab_bytes);
    s->history.resize(max_batch);
    for (auto &h : s->history) h.reserve((size_t)o.max_cycles + 1);
    return s;
}

int mg_batch_solver_solve(mg_batch_solver *s, int n, const double *const *F_dev, double *const *U_dev, mg_solve_result *out,
                          mg_batch_solve_stats *stats)
{
    mg_batch_solve_stats bs;
    std::memset(&bs, 0, sizeof bs);
    std::vector<mg_solve_result> r(n > 0 ? (size_t)n : 0);
    for (auto &x : r) std::memset(&x, 0, sizeof x);
    auto finish = [&](int status) {
        if (out && s && n >= 1 && n <= s->max_batch) {
            for (int i = 0; i < n; ++i) {
                if (status > 0) r[i].status = status;
                r[i].device_ms = bs.device_ms;
                r[i].n_history = (int)s->history[i].size();
                r[i].history = s->history[i].empty() ? nullptr : s->history[i].data();
                out[i] = r[i];
            }
        }
        if (stats) *stats = bs;
        return status;
    };
    if (!require_ready("mg_batch_solver_solve")) return finish(MG_ERR_NOT_INIT);
    if (!s || !F_dev || !U_dev || !out) {
        fail(MG_ERR_ARG, "mg_batch_solver_solve: NULL solver, array or result array");
        return finish(MG_ERR_ARG);
    }
    if (n < 1 || n > s->max_batch) {
        fail(MG_ERR_ARG, "mg_batch_solver_solve: n = %d outside [1, max_batch = %d]", n, s->max_batch);
        return finish(MG_ERR_ARG);
    }
    if (s->n_coef > 1 && n > s->n_coef) {
        fail(MG_ERR_ARG, "mg_batch_solver_solve: n = %d instances, but the solver holds %d coefficients (one per instance)", n, s->n_coef);
        return finish(MG_ERR_ARG);
    }
    if (s->n_react > 1 && n > s->n_react) {
        fail(MG_ERR_ARG, "mg_batch_solver_solve: n = %d instances, but the solver holds %d reaction terms (one per instance)", n, s->n_react);
        return finish(MG_ERR_ARG);
    }
    for (int i = 0; i < n; ++i) s->history[i].clear();
    if (!instances_ok("mg_batch_solver_solve", s, n, F_dev, U_dev)) return finish(MG_ERR_ARG);
    std::vector<int> all(n);
    for (int i = 0; i < n; ++i) all[i] = i;
    return finish(solve_instances(s, n, F_dev, U_dev, all, r, bs));
}

void mg_batch_solver_destroy(mg_batch_solver *s)
{
    if (!s) return;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    release(s);
}

// ------------------------------------------------------------------ variable coefficient (include/mg_varcoef_batch.h)
int mg_batch_solver_set_coefficient(mg_batch_solver *s, int n, const double *const *a_dev)
{
    if (!require_ready("mg_batch_solver_set_coefficient")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_coefficient: NULL solver");
        return MG_ERR_ARG;
    }
    if (n < 0 || n > s->max_batch) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_coefficient: n = %d outside [0, max_batch = %d]", n, s->max_batch);
        return MG_ERR_ARG;
    }
    if (n == 0) {
        if (a_dev) {
            fail(MG_ERR_ARG, "mg_batch_solver_set_coefficient: n = 0 takes the coefficient away and needs a NULL array");
            return MG_ERR_ARG;
        }
        s->n_coef = 0;   // back to the constant-coefficient solver (the level storage stays for the next coefficient)
        return MG_OK;
    }
    if (!a_dev) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_coefficient: NULL array of %d coefficients", n);
        return MG_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (!a_dev[i] || (uintptr_t)a_dev[i] % 16 != 0) {
            fail(MG_ERR_ARG, "mg_batch_solver_set_coefficient: the coefficient of instance %d is NULL or not 16-byte aligned", i);
            return MG_ERR_ARG;
        }
    const hipStream_t st = ctx().stream;
    const int nl = (int)s->sizes.size(), mb = s->max_batch;
    if (!s->coef_flags &&
        !(MG_HIP(hipMalloc((void **)&s->coef_flags, mb * sizeof(int))) &&
          MG_HIP(hipHostMalloc((void **)&s->host_coef_flags, mb * sizeof(int), hipHostMallocDefault)))) {
        if (s->coef_flags) { (void)hipFree(s->coef_flags); s->coef_flags = nullptr; }
        return MG_ERR_HIP;
    }
    // level storage for n instances: what is there when it is large enough, else a fresh set, which replaces the old one
    // only once the check has passed -- a refused coefficient leaves the solver's own untouched
    std::vector<double *> fresh;
    auto drop_fresh = [&]() {
        for (double *p : fresh) if (p) (void)hipFree(p);
        fresh.clear();
    };
    if (s->coef_cap < n) {
        fresh.assign(nl, nullptr);
        for (int l = 0; l < nl; ++l)
            if (!MG_HIP(hipMalloc((void **)&fresh[l], s->pitch[l] * n * sizeof(double)))) {
                drop_fresh();
                return MG_ERR_HIP;
            }
    }
    const std::vector<double *> &dst = fresh.empty() ? s->coef : fresh;
    // tables: the check and the copy into level 0 (slot 0: in = the caller's a_i, out = level 0), then per level the
    // coarsening (slot 1 + l: in = level l, out = level l + 1).  The solver's own tables: every solve rebuilds them.
    for (int i = 0; i < n; ++i) {
        s->host_tab[i] = NodeBatchItem{a_dev[i], nullptr, nullptr, dst[0] + (size_t)i * s->pitch[0], nullptr};
        for (int l = 0; l + 1 < nl; ++l)
            s->host_tab[(size_t)(1 + l) * mb + i] =
                NodeBatchItem{dst[l] + (size_t)i * s->pitch[l], nullptr, nullptr, dst[l + 1] + (size_t)i * s->pitch[l + 1], nullptr};
    }
    const size_t n0 = (size_t)s->N * s->N;
    bool ok = MG_HIP(hipMemcpyAsync(s->dev_tab, s->host_tab, (size_t)nl * mb * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)) &&
              MG_HIP(hipMemsetAsync(s->coef_flags, 0, n * sizeof(int), st));
    if (ok) {
        // the check comes first and reads the CALLER's arrays
        k::coef_check_batch(st, n, n0, s->dev_tab, s->coef_flags);
        ok = MG_HIP(hipMemcpyAsync(s->host_coef_flags, s->coef_flags, n * sizeof(int), hipMemcpyDeviceToHost, st)) &&
             MG_HIP(hipStreamSynchronize(st));
    }
    if (!ok) {
        drop_fresh();
        return MG_ERR_HIP;
    }
    for (int i = 0; i < n; ++i)
        if (s->host_coef_flags[i]) {
            drop_fresh();
            fail(MG_ERR_ARG, "mg_batch_solver_set_coefficient: every value of a must be finite and > 0 (instance %d has one that is not)", i);
            return MG_ERR_ARG;
        }
    // from here on the level storage is overwritten: until it is whole again the solver has NO coefficient, so a HIP error
    // below leaves the constant-coefficient solver, never one on a half-replaced coefficient
    s->n_coef = 0;
    if (!fresh.empty()) {
        for (double *p : s->coef) if (p) (void)hipFree(p);
        s->coef.swap(fresh);
        fresh.clear();
        s->coef_cap = n;
    }
    k::copy_batch(st, n, n0, s->dev_tab);
    for (int l = 0; l + 1 < nl; ++l)
        k::coef_coarsen_batch(st, n, s->sizes[l], s->sizes[l + 1], s->dev_tab + (size_t)(1 + l) * mb,
                              restrict_table(s->sizes[l], s->sizes[l + 1]));
    if (!MG_HIP(hipStreamSynchronize(st))) return MG_ERR_HIP;   // (the caller may free the a_i, or solve on another stream)
    s->n_coef = n;
    return MG_OK;
}

int mg_batch_solver_has_coefficient(const mg_batch_solver *s) { return s ? s->n_coef : 0; }

// ------------------------------------------------------------------ variable reaction term (include/mg_rx_batch.h)
// mg_batch_solver_set_coefficient's steps with the reaction's check (>= 0) and storage of its own
int mg_batch_solver_set_reaction(mg_batch_solver *s, int n, const double *const *s_dev)
{
    if (!require_ready("mg_batch_solver_set_reaction")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_reaction: NULL solver");
        return MG_ERR_ARG;
    }
    if (n < 0 || n > s->max_batch) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_reaction: n = %d outside [0, max_batch = %d]", n, s->max_batch);
        return MG_ERR_ARG;
    }
    if (n == 0) {
        if (s_dev) {
            fail(MG_ERR_ARG, "mg_batch_solver_set_reaction: n = 0 takes the reaction away and needs a NULL array");
            return MG_ERR_ARG;
        }
        s->n_react = 0;   // the solver without a reaction again (the level storage stays for the next one)
        return MG_OK;
    }
    if (!s_dev) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_reaction: NULL array of %d reaction terms", n);
        return MG_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (!s_dev[i] || (uintptr_t)s_dev[i] % 16 != 0) {
            fail(MG_ERR_ARG, "mg_batch_solver_set_reaction: the reaction term of instance %d is NULL or not 16-byte aligned", i);
            return MG_ERR_ARG;
        }
    const hipStream_t st = ctx().stream;
    const int nl = (int)s->sizes.size(), mb = s->max_batch;
    if (!s->coef_flags &&
        !(MG_HIP(hipMalloc((void **)&s->coef_flags, mb * sizeof(int))) &&
          MG_HIP(hipHostMalloc((void **)&s->host_coef_flags, mb * sizeof(int), hipHostMallocDefault)))) {
        if (s->coef_flags) { (void)hipFree(s->coef_flags); s->coef_flags = nullptr; }
        return MG_ERR_HIP;
    }
    // level storage for n instances: what is there when it is large enough, else a fresh set, which replaces the old one
    // only once the check has passed -- a refused reaction leaves the solver's own untouched
    std::vector<double *> fresh;
    auto drop_fresh = [&]() {
        for (double *p : fresh) if (p) (void)hipFree(p);
        fresh.clear();
    };
    if (s->react_cap < n) {
        fresh.assign(nl, nullptr);
        for (int l = 0; l < nl; ++l)
            if (!MG_HIP(hipMalloc((void **)&fresh[l], s->pitch[l] * n * sizeof(double)))) {
                drop_fresh();
                return MG_ERR_HIP;
            }
    }
    const std::vector<double *> &dst = fresh.empty() ? s->react : fresh;
    // tables: the check and the copy into level 0 (slot 0: in = the caller's s_i, out = level 0), then per level the
    // coarsening (slot 1 + l: in = level l, out = level l + 1).  The solver's own tables: every solve rebuilds them.
    for (int i = 0; i < n; ++i) {
        s->host_tab[i] = NodeBatchItem{s_dev[i], nullptr, nullptr, dst[0] + (size_t)i * s->pitch[0], nullptr};
        for (int l = 0; l + 1 < nl; ++l)
            s->host_tab[(size_t)(1 + l) * mb + i] =
                NodeBatchItem{dst[l] + (size_t)i * s->pitch[l], nullptr, nullptr, dst[l + 1] + (size_t)i * s->pitch[l + 1], nullptr};
    }
    const size_t n0 = (size_t)s->N * s->N;
    bool ok = MG_HIP(hipMemcpyAsync(s->dev_tab, s->host_tab, (size_t)nl * mb * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)) &&
              MG_HIP(hipMemsetAsync(s->coef_flags, 0, n * sizeof(int), st));
    if (ok) {
        // the check comes first and reads the CALLER's arrays
        k::reaction_check_batch(st, n, n0, s->dev_tab, s->coef_flags);
        ok = MG_HIP(hipMemcpyAsync(s->host_coef_flags, s->coef_flags, n * sizeof(int), hipMemcpyDeviceToHost, st)) &&
             MG_HIP(hipStreamSynchronize(st));
    }
    if (!ok) {
        drop_fresh();
        return MG_ERR_HIP;
    }
    for (int i = 0; i < n; ++i)
        if (s->host_coef_flags[i]) {
            drop_fresh();
            fail(MG_ERR_ARG, "mg_batch_solver_set_reaction: every value of s must be finite and >= 0 (instance %d has one that is not)", i);
            return MG_ERR_ARG;
        }
    // from here on the level storage is overwritten: until it is whole again the solver has NO reaction, so a HIP error
    // below never leaves a solver on a half-replaced term
    s->n_react = 0;
    if (!fresh.empty()) {
        for (double *p : s->react) if (p) (void)hipFree(p);
        s->react.swap(fresh);
        fresh.clear();
        s->react_cap = n;
    }
    k::copy_batch(st, n, n0, s->dev_tab);
    for (int l = 0; l + 1 < nl; ++l)
        k::coef_coarsen_batch(st, n, s->sizes[l], s->sizes[l + 1], s->dev_tab + (size_t)(1 + l) * mb,
                              restrict_table(s->sizes[l], s->sizes[l + 1]));
    if (!MG_HIP(hipStreamSynchronize(st))) return MG_ERR_HIP;   // (the caller may free the s_i, or solve on another stream)
    s->n_react = n;
    return MG_OK;
}

int mg_batch_solver_has_reaction(const mg_batch_solver *s) { return s ? s->n_react : 0; }

// ------------------------------------------------------------------ semilinear problem (include/mg_newton_batch.h)
int mg_batch_solver_newton(mg_batch_solver *s, int n, int kind, const double *kappa, int n_w, const double *const *w_dev,
                           const double *const *F_dev, double *const *U_dev, const mg_newton_opts *opts, mg_newton_result *out,
                           mg_batch_newton_stats *stats)
{
    const char *who = "mg_batch_solver_newton";
    mg_batch_newton_stats ns;
    std::memset(&ns, 0, sizeof ns);
    std::vector<mg_newton_result> r(n > 0 ? (size_t)n : 0);
    for (auto &x : r) std::memset(&x, 0, sizeof x);
    auto finish = [&](int status) {
        if (out && s && n >= 1 && n <= s->max_batch)
            for (int i = 0; i < n; ++i) {
                if (status > 0) r[i].status = status;
                r[i].n_history = i < s->nw_n ? (int)s->nw_hist[i].size() : 0;
                out[i] = r[i];
            }
        if (stats) *stats = ns;
        return status;
    };
    if (!require_ready(who)) return finish(MG_ERR_NOT_INIT);
    if (!s || !kappa || !F_dev || !U_dev) {
        fail(MG_ERR_ARG, "%s: NULL solver, kappa or array", who);
        return finish(MG_ERR_ARG);
    }
    if (s->n_react > 0) {
        fail(MG_ERR_UNSUPPORTED, "%s: a reaction term is set; the driver installs the Newton matrices' own (take yours away with "
                                 "mg_batch_solver_set_reaction(s, 0, NULL), or put it into w)", who);
        return finish(MG_ERR_UNSUPPORTED);
    }
    if (n < 1 || n > s->max_batch) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, max_batch = %d]", who, n, s->max_batch);
        return finish(MG_ERR_ARG);
    }
    if (s->n_coef > 1 && n > s->n_coef) {
        fail(MG_ERR_ARG, "%s: n = %d instances, but the solver holds %d coefficients (one per instance)", who, n, s->n_coef);
        return finish(MG_ERR_ARG);
    }
    if (!optional_arrays_ok(who, "w", n, n_w, w_dev) || !newton_kind_ok(who, kind) || !kappas_ok(who, n, kappa) ||
        !instances_ok(who, s, n, F_dev, U_dev))
        return finish(MG_ERR_ARG);
    mg_newton_opts o;
    mg_newton_opts_default(&o);
    if (opts) o = *opts;
    if (!(o.rtol >= 0.0) || !(o.atol >= 0.0) || !std::isfinite(o.rtol) || !std::isfinite(o.atol) || o.max_iters < 0 || o.max_backtracks < 0) {
        fail(MG_ERR_ARG, "%s: rtol = %g, atol = %g (non-negative, finite), max_iters = %d, max_backtracks = %d (>= 0 each)", who, o.rtol,
             o.atol, o.max_iters, o.max_backtracks);
        return finish(MG_ERR_ARG);
    }
    const hipStream_t st = ctx().stream;
    const int N = s->N, nl = (int)s->sizes.size(), mb = s->max_batch;
    const size_t n0 = (size_t)N * N, p0 = s->pitch[0];
    const bool has_a = s->n_coef > 0, has_w = n_w > 0;
    if (!newton_storage(s)) return finish(MG_ERR_HIP);
    if (has_w) {   // one launch over the n_w arrays, a flag each, one read-back, as mg_batch_solver_set_reaction checks s
        for (int i = 0; i < n_w; ++i) s->host_tab[i] = NodeBatchItem{w_dev[i], nullptr, nullptr, nullptr, nullptr};
        if (!MG_HIP(hipMemcpyAsync(s->dev_tab, s->host_tab, (size_t)n_w * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)) ||
            !MG_HIP(hipMemsetAsync(s->coef_flags, 0, n_w * sizeof(int), st)))
            return finish(MG_ERR_HIP);
        k::reaction_check_batch(st, n_w, n0, s->dev_tab, s->coef_flags);
        ns.launches += 1;
        if (!MG_HIP(hipMemcpyAsync(s->host_coef_flags, s->coef_flags, n_w * sizeof(int), hipMemcpyDeviceToHost, st)) ||
            !MG_HIP(hipStreamSynchronize(st)))
            return finish(MG_ERR_HIP);
        for (int i = 0; i < n_w; ++i)
            if (s->host_coef_flags[i]) {
                fail(MG_ERR_ARG, "%s: every value of w must be finite and >= 0 (instance %d has one that is not)", who, i);
                return finish(MG_ERR_ARG);
            }
    }
    // From here on the call's records replace the last call's.  Per instance: cur holds the last accepted iterate, D its
    // right-hand side and S its Newton matrix's term; oth, D2 and S2 take the next trial.  U_dev[i] is one of (cur, oth): when
    // the instance ends on the other one, the iterate is copied home.
    struct Inst {
        double *cur, *oth, *D, *D2, *S, *S2, *dlt;
        double rn, tol;
        bool stalled;
    };
    std::vector<Inst> in(n);
    s->nw_n = n;
    for (int i = 0; i < n; ++i) {
        s->nw_hist[i].clear();
        s->history[i].clear();
        in[i] = Inst{U_dev[i], s->nw_field + (0 * (size_t)mb + i) * p0, s->nw_field + (1 * (size_t)mb + i) * p0,
                     s->nw_field + (2 * (size_t)mb + i) * p0, level(s, s->react, 0, i), s->nw_field + (3 * (size_t)mb + i) * p0,
                     s->nw_field + (4 * (size_t)mb + i) * p0, 0.0, 0.0, false};
    }
    if (s->kr_m > 0) {
        s->kr_n = n;
        for (int i = 0; i < n; ++i) {
            s->kr_records[i] = 0;
            s->kr_brk[i] = 0;
        }
    }
    const LevelConsts &c0 = s->lc[0];
    const NewtonBlock host = newton_block(s->nw_host, nl, mb), dev = newton_block(s->nw_dev, nl, mb);
    auto coef_of = [&](int i) -> const double * { return has_a ? level(s, s->coef, 0, s->n_coef == 1 ? 0 : i) : nullptr; };
    // the pass over the instances `sub` (step: the trial at t into the second set), their norms into host.norms by slot
    auto pass = [&](const std::vector<int> &sub, bool step, double t) {
        const int m = (int)sub.size();
        for (int j = 0; j < m; ++j) {
            const Inst &x = in[sub[j]];
            host.pass[j] = k::NewtonBatchItem{coef_of(sub[j]), has_w ? w_dev[n_w == 1 ? 0 : sub[j]] : nullptr, x.cur, step ? x.dlt : nullptr,
                                              F_dev[sub[j]], step ? x.oth : nullptr, step ? x.D2 : x.D, step ? x.S2 : x.S, kappa[sub[j]]};
        }
        if (!MG_HIP(hipMemcpyAsync(dev.pass, host.pass, (size_t)m * sizeof(k::NewtonBatchItem), hipMemcpyHostToDevice, st))) return false;
        k::newton_residual_batch(st, m, N, c0.inv, c0.sd, kind, has_a, has_w, step, t, dev.pass, s->part, dev.norms);
        ns.launches += 2;
        return MG_HIP(hipMemcpyAsync(host.norms, dev.norms, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st)) &&
               MG_HIP(hipEventRecord(s->ev_sync, st)) && MG_HIP(hipEventSynchronize(s->ev_sync));
    };
    // every instance whose accepted iterate sits in solver storage goes home in one launch
    auto home = [&]() {
        int m = 0;
        for (int i = 0; i < n; ++i)
            if (in[i].cur != U_dev[i]) host.coarsen[m++] = NodeBatchItem{in[i].cur, nullptr, nullptr, U_dev[i], nullptr};
        if (m == 0) return true;
        if (!MG_HIP(hipMemcpyAsync(dev.coarsen, host.coarsen, (size_t)m * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st))) return false;
        k::copy_batch(st, m, n0, dev.coarsen);
        ns.launches += 1;
        return MG_HIP(hipStreamSynchronize(st));
    };
    if (!MG_HIP(hipEventRecord(s->nw_ev_begin, st))) return finish(MG_ERR_HIP);
    std::vector<int> act(n), next, pending;
    for (int i = 0; i < n; ++i) act[i] = i;
    if (!pass(act, false, 0.0)) return finish(MG_ERR_HIP);
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(host.norms[i])) {
            fail(MG_ERR_ARG, "%s: the residual of the start of instance %d is not finite (%g)", who, i, host.norms[i]);
            return finish(MG_ERR_ARG);
        }
    next.clear();
    for (int i = 0; i < n; ++i) {
        in[i].rn = r[i].res0 = r[i].res = host.norms[i];
        in[i].tol = std::fmax(o.atol, o.rtol * in[i].rn);
        if (!(in[i].rn <= in[i].tol) && o.max_iters > 0) next.push_back(i);
    }
    act.swap(next);
    std::vector<const double *> Dp(n, nullptr);
    std::vector<double *> dl(n, nullptr);
    std::vector<mg_solve_result> inner(n);
    std::vector<mg_newton_iter> it(n);
    for (int i = 0; i < n; ++i) dl[i] = in[i].dlt;
    while (!act.empty()) {
        const int na = (int)act.size();
        for (int j = 0; j < na; ++j) {
            const int i = act[j];
            for (int l = 0; l + 1 < nl; ++l)
                host.coarsen[(size_t)l * mb + j] =
                    NodeBatchItem{l == 0 ? in[i].S : level(s, s->react, l, i), nullptr, nullptr, level(s, s->react, l + 1, i), nullptr};
            s->nw_S0[i] = in[i].S;
            Dp[i] = in[i].D;
            std::memset(&inner[i], 0, sizeof inner[i]);
            s->history[i].clear();
        }
        int status = MG_OK;
        if (nl > 1 && !MG_HIP(hipMemcpyAsync(dev.coarsen, host.coarsen, (size_t)(nl - 1) * mb * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)))
            status = MG_ERR_HIP;
        if (status == MG_OK) {
            for (int l = 0; l + 1 < nl; ++l)
                k::coef_coarsen_batch(st, na, s->sizes[l], s->sizes[l + 1], dev.coarsen + (size_t)l * mb,
                                      restrict_table(s->sizes[l], s->sizes[l + 1]));
            ns.launches += nl - 1;
            // (the delta of all n instances are one region: one memset, whatever the number that still iterate)
            if (!MG_HIP(hipMemsetAsync(s->nw_field + 4 * (size_t)mb * p0, 0, (size_t)n * p0 * sizeof(double), st))) status = MG_ERR_HIP;
        }
        if (status == MG_OK) {
            mg_batch_solve_stats bs;
            std::memset(&bs, 0, sizeof bs);
            s->n_react = n;   // the driver's own per-instance reaction, for the length of the inner solve
            s->nw_on = true;
            status = solve_instances(s, n, Dp.data(), dl.data(), act, inner, bs);
            s->nw_on = false;
            s->n_react = 0;
            ns.launches += bs.launches;
            ns.inner_cycles += bs.cycles;
        }
        if (status > 0) {
            (void)home();
            return finish(status);
        }
        for (int i : act) {
            it[i] = mg_newton_iter{in[i].rn, 0.0, 0, inner[i].cycles, inner[i].converged, inner[i].coarse_capped};
            r[i].inner_cycles += inner[i].cycles;
        }
        // the line search in rounds: round k is one launch at t = 2^-k over the instances that have not accepted yet
        pending = act;
        next.clear();
        double t = 1.0;
        while (!pending.empty()) {
            if (!pass(pending, true, t)) {
                (void)home();
                return finish(MG_ERR_HIP);
            }
            ns.trial_rounds += 1;
            std::vector<int> again;
            for (size_t j = 0; j < pending.size(); ++j) {
                const int i = pending[j];
                Inst &x = in[i];
                const double rt = host.norms[j];
                r[i].trials += 1;
                if (std::isfinite(rt) && rt < (1.0 - 1e-4 * t) * x.rn) {
                    std::swap(x.cur, x.oth);
                    std::swap(x.D, x.D2);
                    std::swap(x.S, x.S2);
                    x.rn = rt;
                    it[i].res = rt;
                    it[i].t = t;
                    s->nw_hist[i].push_back(it[i]);
                    r[i].iterations += 1;
                    if (r[i].iterations > ns.iterations) ns.iterations = r[i].iterations;
                    continue;
                }
                it[i].backtracks += 1;
                if (it[i].backtracks > o.max_backtracks) {
                    s->nw_hist[i].push_back(it[i]);
                    x.stalled = true;
                } else {
                    again.push_back(i);
                }
            }
            pending.swap(again);
            t *= 0.5;
        }
        for (int i : act)
            if (!in[i].stalled && !(in[i].rn <= in[i].tol) && r[i].iterations < o.max_iters) next.push_back(i);
        act.swap(next);
    }
    if (!home()) return finish(MG_ERR_HIP);
    if (!MG_HIP(hipEventRecord(s->nw_ev_end, st)) || !MG_HIP(hipEventSynchronize(s->nw_ev_end))) return finish(MG_ERR_HIP);
    float ms = 0.0f;
    if (MG_HIP(hipEventElapsedTime(&ms, s->nw_ev_begin, s->nw_ev_end))) ns.device_ms = ms;
    bool all = true;
    for (int i = 0; i < n; ++i) {
        r[i].res = in[i].rn;
        r[i].converged = in[i].rn <= in[i].tol ? 1 : 0;
        r[i].status = r[i].converged ? MG_NEWTON_CONVERGED : in[i].stalled ? MG_NEWTON_STALLED : MG_NEWTON_NOT_CONVERGED;
        all = all && r[i].converged;
    }
    return finish(all ? MG_NEWTON_CONVERGED : MG_NEWTON_NOT_CONVERGED);
}

int mg_batch_solver_newton_history(const mg_batch_solver *s, int i, mg_newton_iter *out, int cap)
{
    if (!s || i < 0 || i >= s->nw_n) return 0;
    const int n = (int)s->nw_hist[i].size();
    for (int j = 0; out && j < n && j < cap; ++j) out[j] = s->nw_hist[i][j];
    return n;
}

int mg_batch_solver_newton_inner_history(const mg_batch_solver *s, int i, double *out, int cap)
{
    if (!s || i < 0 || i >= s->nw_n) return 0;
    const int n = (int)s->history[i].size();
    for (int j = 0; out && j < n && j < cap; ++j) out[j] = s->history[i][j];
    return n;
}

int mg_nonlinearResidual_batch(int n, int N, double L, double shift, int n_a, const double *const *a_dev, int kind, const double *kappa,
                               int n_w, const double *const *w_dev, const double *const *U, const double *const *dlt, double t,
                               const double *const *F, double *const *V, double *const *D, double *const *S, double *norms_out)
{
    const char *who = "mg_nonlinearResidual_batch";
    if (!require_ready(who)) return MG_ERR_NOT_INIT;
    if (n < 1 || n > 65535 || N < 3 || !(L > 0.0) || !std::isfinite(L) || !(shift >= 0.0) || !std::isfinite(shift)) {
        fail(MG_ERR_ARG, "%s: n = %d inside [1, 65535], N = %d (at least 3), L = %g (positive, finite), shift = %g (finite, >= 0)", who, n, N,
             L, shift);
        return MG_ERR_ARG;
    }
    if (!kappa || !U || !F || !D || !S || (dlt && (!V || !std::isfinite(t)))) {
        fail(MG_ERR_ARG, "%s: NULL kappa, U, F, D or S; with dlt, V must be there and t = %g finite", who, t);
        return MG_ERR_ARG;
    }
    if (!optional_arrays_ok(who, "a", n, n_a, a_dev) || !optional_arrays_ok(who, "w", n, n_w, w_dev) || !newton_kind_ok(who, kind) ||
        !kappas_ok(who, n, kappa))
        return MG_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const bool there = U[i] && F[i] && D[i] && S[i] && (!dlt || (dlt[i] && V[i]));
        const uintptr_t bits = (uintptr_t)U[i] | (uintptr_t)F[i] | (uintptr_t)D[i] | (uintptr_t)S[i] |
                               (dlt && there ? (uintptr_t)dlt[i] | (uintptr_t)V[i] : 0);
        if (!there || bits % 16 != 0) {
            fail(MG_ERR_ARG, "%s: a NULL or not 16-byte aligned array of instance %d", who, i);
            return MG_ERR_ARG;
        }
    }
    const hipStream_t st = ctx().stream;
    const size_t np = k::resnorm_partials(N);
    const double dx = L / (double)(N - 1), dx2 = dx * dx;
    std::vector<k::NewtonBatchItem> items(n);
    for (int i = 0; i < n; ++i)
        items[i] = k::NewtonBatchItem{n_a ? a_dev[n_a == 1 ? 0 : i] : nullptr, n_w ? w_dev[n_w == 1 ? 0 : i] : nullptr, U[i],
                                      dlt ? dlt[i] : nullptr, F[i], dlt ? V[i] : nullptr, D[i], S[i], kappa[i]};
    k::NewtonBatchItem *tab = nullptr;
    double *buf = nullptr;   // the partials of every instance and, behind them, the n norms
    if (!MG_HIP(hipMalloc((void **)&tab, (size_t)n * sizeof(k::NewtonBatchItem)))) return MG_ERR_HIP;
    if (!MG_HIP(hipMalloc((void **)&buf, ((size_t)n * np + n) * sizeof(double)))) {
        (void)hipFree(tab);
        return MG_ERR_HIP;
    }
    std::vector<double> host(n, 0.0);
    bool ok = MG_HIP(hipMemcpyAsync(tab, items.data(), (size_t)n * sizeof(k::NewtonBatchItem), hipMemcpyHostToDevice, st)) &&
              MG_HIP(hipStreamSynchronize(st));   // (items is pageable host memory of this frame)
    if (ok) {
        // (timed for scripts/bench_newton_batched.py: the bytes of mg_nonlinearResidual's scope, times n)
        const double pts = (double)N * N * n;
        ProfScope ps(dlt ? "newton_step_batch" : "newton_residual_batch", N, pts * (32.0 + (n_a ? 8.0 : 0.0) + (n_w ? 8.0 : 0.0) + (dlt ? 16.0 : 0.0)));
        k::newton_residual_batch(st, n, N, 1.0 / dx2, shift * dx2, kind, n_a > 0, n_w > 0, dlt != nullptr, t, tab, buf, buf + (size_t)n * np);
    }
    ok = ok && MG_HIP(hipMemcpyAsync(host.data(), buf + (size_t)n * np, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st)) &&
         MG_HIP(hipStreamSynchronize(st));
    (void)hipFree(tab);
    (void)hipFree(buf);
    if (!ok) return MG_ERR_HIP;
    for (int i = 0; norms_out && i < n; ++i) norms_out[i] = host[i];
    return MG_OK;
}

// ------------------------------------------------------------------ Krylov acceleration (include/mg_krylov_batch.h)
int mg_batch_solver_set_krylov(mg_batch_solver *s, int m)
{
    if (!require_ready("mg_batch_solver_set_krylov")) return MG_ERR_NOT_INIT;
    if (!s || m < 0 || m > MG_KRYLOV_MAX_M) {
        fail(MG_ERR_ARG, "mg_batch_solver_set_krylov: NULL solver, or m = %d outside [0, %d]", m, MG_KRYLOV_MAX_M);
        return MG_ERR_ARG;
    }
    const int have = (int)s->kr_Z.size(), mb = s->max_batch;
    if (m > have) {   // the additional slots, and with the first of them r, the partials, the scalars, the log and the tables
        const size_t n_field = s->pitch[0] * mb;
        const size_t n_part = (size_t)k::KRYLOV_MAX_K * k::krylov_blocks(s->N) * mb;
        const size_t n_scal = (size_t)k::KRYLOV_SCAL_COUNT * mb, n_log = krylov_log_stride(s) * mb;
        const bool first = s->kr_r == nullptr;
        auto dev_alloc = [](double **p, size_t count) { return MG_HIP(hipMalloc((void **)p, count * sizeof(double))); };
        std::vector<double *> Z, Q;
        double *r = nullptr, *part = nullptr, *scal = nullptr, *log = nullptr, *rb = nullptr, *host_rb = nullptr;
        void *dev_tab = nullptr, *host_tab = nullptr;
        bool ok = true;
        if (first)
            ok = dev_alloc(&r, n_field) && dev_alloc(&part, n_part) && dev_alloc(&scal, n_scal) && dev_alloc(&log, n_log) &&
                 dev_alloc(&rb, 2 * (size_t)mb) && MG_HIP(hipMalloc(&dev_tab, krylov_tables_bytes(mb))) &&
                 MG_HIP(hipHostMalloc((void **)&host_rb, 2 * (size_t)mb * sizeof(double), hipHostMallocDefault)) &&
                 MG_HIP(hipHostMalloc(&host_tab, krylov_tables_bytes(mb), hipHostMallocDefault)) &&
                 MG_HIP(hipMemset(scal, 0, n_scal * sizeof(double))) && MG_HIP(hipMemset(rb, 0, 2 * (size_t)mb * sizeof(double)));
        for (int j = have; j < m && ok; ++j) {
            double *z = nullptr, *q = nullptr;
            ok = dev_alloc(&z, n_field);
            if (ok) Z.push_back(z);
            ok = ok && dev_alloc(&q, n_field);
            if (ok) Q.push_back(q);
        }
        if (!ok) {   // the solver keeps what it had
            for (double *p : Z) (void)hipFree(p);
            for (double *p : Q) (void)hipFree(p);
            for (double *p : {r, part, scal, log, rb}) if (p) (void)hipFree(p);
            if (dev_tab) (void)hipFree(dev_tab);
            if (host_rb) (void)hipHostFree(host_rb);
            if (host_tab) (void)hipHostFree(host_tab);
            return MG_ERR_HIP;
        }
        if (pool_poison_wanted()) {   // MG_POOL_POISON: no array starts from what hipMalloc happened to return
            for (double *p : Z) poison_block(p, n_field * sizeof(double));
            for (double *p : Q) poison_block(p, n_field * sizeof(double));
            if (first) {
                poison_block(r, n_field * sizeof(double));
                poison_block(part, n_part * sizeof(double));
                poison_block(log, n_log * sizeof(double));
            }
            (void)MG_HIP(hipStreamSynchronize(ctx().stream));
        }
        if (first) {
            s->kr_r = r;
            s->kr_part = part;
            s->kr_scal = scal;
            s->kr_log = log;
            s->kr_rb = rb;
            s->kr_host_rb = host_rb;
            s->kr_dev_tab = dev_tab;
            s->kr_host_tab = host_tab;
            std::memset(host_tab, 0, krylov_tables_bytes(mb));
            std::memset(host_rb, 0, 2 * (size_t)mb * sizeof(double));
            s->kr_log_host.assign(n_log, 0.0);
            s->kr_k.assign(mb, 0);
            s->kr_records.assign(mb, 0);
            s->kr_brk.assign(mb, 0);
            s->kr_F.assign(mb, nullptr);
            s->kr_U.assign(mb, nullptr);
        }
        s->kr_Z.insert(s->kr_Z.end(), Z.begin(), Z.end());
        s->kr_Q.insert(s->kr_Q.end(), Q.begin(), Q.end());
    }
    s->kr_m = m;
    return MG_OK;
}

int mg_batch_solver_krylov(const mg_batch_solver *s) { return s ? s->kr_m : 0; }

int mg_batch_solver_krylov_breakdown(const mg_batch_solver *s, int i)
{
    return s && s->kr_m > 0 && i >= 0 && i < s->kr_n && s->kr_brk[i] ? 1 : 0;
}

int mg_batch_solver_krylov_log(const mg_batch_solver *s, int i, double *out, int cap)
{
    if (!s || i < 0 || i >= s->kr_n) return 0;
    const int have = s->kr_records[i];
    if (!out) return have;
    const int n = cap < have ? (cap > 0 ? cap : 0) : have;
    if (n > 0)
        std::memcpy(out, s->kr_log_host.data() + (size_t)i * krylov_log_stride(s), (size_t)n * (s->kr_log_m + 7) * sizeof(double));
    return n;
}

}  // extern "C"
