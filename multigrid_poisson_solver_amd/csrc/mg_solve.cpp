// mg_solve.cpp -- residual-tolerance solver (include/mg_hip.h, "residual-tolerance solver"): V(pre, post) cycles on a
// caller's F and Dirichlet rim until the interior L2 residual meets the tolerance.  One cycle follows the reference
// driver's node order (src/MG_solver_CPU.cpp:259-416) with the weighted Jacobi smoother and the relative coarse target
// of mg_solve_kernels.hip; the transfer operators are the engine's own (mg_kernels.hip).  A driver of its own, not a mode
// of the cycle-file interpreter (mg_cycle.cpp): every level array is allocated at creation, a solve allocates nothing.
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "mg_internal.h"

using namespace mg;

struct mg_solver {
    int N = 0;
    double L = 1.0;
    mg_solve_opts o{};
    std::vector<int> sizes;                  // N, N/2, ... >= N_min
    std::vector<LevelConsts> lc;             // per level: spacing, centre coefficient, weight
    std::vector<double *> A, B, F;           // per level (level 0: only B, the scratch field beside the caller's U)
    SolveLevels lv{};                        // the vectors above and the coarse solve's slots: set at creation
    // the operator of the levels: set at creation; op.coef (&coef, or nullptr: none is set) and op.kind (bc, or nullptr: no
    // side is Neumann) are the solver's state, changed by mg_solver_set_coefficient and mg_solver_set_boundary alone
    SolveOperator op{};
    std::vector<SolveCycle> cyc[2];          // [fused][top]: the recorded cycles, top = 0 and (o.fmg >= 1) every level above the last
    double *part = nullptr;                 // norm partials
    double *dev_scal = nullptr;              // [4]: residual norm, reference norm, coarse err0, coarse err
    int *gs_state = nullptr;                 // [4]
    double *host_scal = nullptr;             // pinned [4]
    int *host_state = nullptr;               // pinned [4]
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_norm = nullptr;
    std::vector<double> history;
    // full-multigrid start (o.fmg >= 1; nothing of it is allocated otherwise)
    std::vector<double *> FF;                // per level l >= 1: F_l, the restricted source
    std::vector<double *> G;                 // per level: the rim data g_l as four edges, 4*N_l
    std::vector<k::CubicTable> up, down;     // per level l < last: N_{l+1} -> N_l (prolongation), N_l -> N_{l+1} (rim sampling)
    int *fmg_capped = nullptr;               // device: some coarse solve of the pass ended at its cap
    int *host_fmg_capped = nullptr;          // pinned
    // variable coefficient (include/mg_varcoef.h; nothing of it is allocated before the first mg_solver_set_coefficient)
    std::vector<double *> coef;              // per level: the nodal coefficient a_l
    int *coef_flag = nullptr;                // device: the check found a value that is not finite or not > 0
    int *host_coef_flag = nullptr;           // pinned
    // variable reaction term (include/mg_reaction.h; nothing of it is allocated before the first mg_solver_set_reaction);
    // op.react is &react, or nullptr: none is set
    std::vector<double *> react;             // per level: the nodal reaction term s_l
    int *react_flag = nullptr;               // device: the check found a value that is negative or not finite
    int *host_react_flag = nullptr;          // pinned
    // semilinear driver (include/mg_newton.h; nothing of it is allocated before the first mg_solver_newton)
    double *nw_buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // V, D, D', S', delta: N^2 doubles each
    std::vector<mg_newton_iter> nw_hist;     // the last call's iterations
    // boundary kinds per side (include/mg_bc.h; nothing of it is allocated before the first Neumann side is set)
    int bc[4] = {0, 0, 0, 0};                // S, N, W, E
    std::vector<int *> bc_lo;               // per level l < last: mg_boundary_prolongation_table(N_{l+1}, N_l) on the device
    std::vector<double *> bc_w;
    // the pure Neumann problem (include/mg_singular.h; nothing of it is allocated before the first singular boundary is set).
    // op.project_coarse says whether the boundary that is set is the singular one
    bool mean_on = false;                    // mg_solver_set_mean
    double mean = 0.0;                       // the target of the solution's weighted mean
    double *sing_F = nullptr;                // Ft = F - c_F, N^2
    double *sing_scal = nullptr;             // device [4]: c_F, c_F - 0, mean_w(U), mean_w(U) - mean
    double *sing_host = nullptr;             // pinned [4]
    double sing_info[3] = {0.0, 0.0, 0.0};   // the last solve's c_F, mean_w(U) before the shift, target
    // Krylov acceleration (include/mg_krylov.h; nothing of it is allocated before the first enabling mg_solver_set_krylov)
    int kr_m = 0;                            // 0: off
    double *kr_r = nullptr;                  // the residual r
    std::vector<double *> kr_Z, kr_Q;        // the slots z_j, q_j allocated so far (>= kr_m of each once enabled)
    double *kr_part = nullptr;               // partials: KRYLOV_MAX_K stripes of krylov_blocks(N)
    double *kr_scal = nullptr;               // device [KR_SCALARS]: b_j, w_j, alpha, rho_rec, breakdown
    double *kr_log = nullptr;                // device: max(max_cycles, 1) records of KR_REC_MAX doubles
    double *kr_host = nullptr;               // pinned [2]: rho_rec, breakdown
    std::vector<double> kr_log_host;         // the last solve's records, kr_log_m + 7 doubles each
    int kr_log_m = 0, kr_records = 0;
    bool kr_breakdown = false;
};

namespace {

bool finite(double v) { return std::isfinite(v); }

bool opts_ok(const char *who, int N, double L, const mg_solve_opts &o)
{
    if (!(L > 0.0) || !finite(L)) { fail(MG_ERR_ARG, "%s: L = %g must be positive and finite", who, L); return false; }
    if (o.N_min < 3 || o.N_min > 32) { fail(MG_ERR_ARG, "%s: N_min = %d outside [3, 32]", who, o.N_min); return false; }
    if (N < 2 * o.N_min) {
        fail(MG_ERR_ARG, "%s: N = %d needs at least two levels (N >= 2*N_min = %d)", who, N, 2 * o.N_min);
        return false;
    }
    if (o.pre < 1 || o.pre > 4 || o.post < 1 || o.post > 4) {
        fail(MG_ERR_ARG, "%s: pre = %d / post = %d sweeps outside [1, 4]", who, o.pre, o.post);
        return false;
    }
    if (!(o.omega > 0.0 && o.omega <= 1.0)) { fail(MG_ERR_ARG, "%s: omega = %g outside (0, 1]", who, o.omega); return false; }
    if (!(o.coarse_rtol >= 0.0) || !(o.coarse_atol >= 0.0) || !finite(o.coarse_rtol) || !finite(o.coarse_atol) ||
        !(o.coarse_rtol > 0.0 || o.coarse_atol > 0.0)) {
        fail(MG_ERR_ARG, "%s: coarse_rtol = %g, coarse_atol = %g (non-negative, finite, not both zero)", who, o.coarse_rtol,
             o.coarse_atol);
        return false;
    }
    if (o.coarse_max_iters < 1) { fail(MG_ERR_ARG, "%s: coarse_max_iters = %d < 1", who, o.coarse_max_iters); return false; }
    if (!(o.rtol >= 0.0) || !(o.atol >= 0.0) || !finite(o.rtol) || !finite(o.atol)) {
        fail(MG_ERR_ARG, "%s: rtol = %g, atol = %g must be non-negative and finite", who, o.rtol, o.atol);
        return false;
    }
    if (o.max_cycles < 0) { fail(MG_ERR_ARG, "%s: max_cycles = %d < 0", who, o.max_cycles); return false; }
    // (a negative shift is the indefinite Helmholtz problem: not what this smoother solves)
    if (!(o.shift >= 0.0) || !finite(o.shift)) { fail(MG_ERR_ARG, "%s: shift = %g must be finite and >= 0", who, o.shift); return false; }
    if (o.fmg < 0 || o.fmg > 8) { fail(MG_ERR_ARG, "%s: fmg = %d outside [0, 8]", who, o.fmg); return false; }
    return true;
}

double spacing_sq(int N, double L)
{
    const double dx = L / (double)(N - 1);
    return dx * dx;
}

void release(mg_solver *s)
{
    for (double *p : s->A) if (p) (void)hipFree(p);
    for (double *p : s->B) if (p) (void)hipFree(p);
    for (double *p : s->F) if (p) (void)hipFree(p);
    for (double *p : s->FF) if (p) (void)hipFree(p);
    for (double *p : s->G) if (p) (void)hipFree(p);
    for (auto *v : {&s->up, &s->down})
        for (k::CubicTable &t : *v) {
            if (t.base) (void)hipFree(t.base);
            if (t.w) (void)hipFree(t.w);
        }
    for (double *p : s->coef) if (p) (void)hipFree(p);
    for (int *p : s->bc_lo) if (p) (void)hipFree(p);
    for (double *p : s->bc_w) if (p) (void)hipFree(p);
    if (s->sing_F) (void)hipFree(s->sing_F);
    if (s->sing_scal) (void)hipFree(s->sing_scal);
    if (s->sing_host) (void)hipHostFree(s->sing_host);
    for (double *p : s->react) if (p) (void)hipFree(p);
    for (double *p : s->nw_buf) if (p) (void)hipFree(p);
    if (s->react_flag) (void)hipFree(s->react_flag);
    if (s->host_react_flag) (void)hipHostFree(s->host_react_flag);
    if (s->coef_flag) (void)hipFree(s->coef_flag);
    if (s->host_coef_flag) (void)hipHostFree(s->host_coef_flag);
    for (auto *v : {&s->kr_Z, &s->kr_Q})
        for (double *p : *v) if (p) (void)hipFree(p);
    for (double *p : {s->kr_r, s->kr_part, s->kr_scal, s->kr_log}) if (p) (void)hipFree(p);
    if (s->kr_host) (void)hipHostFree(s->kr_host);
    if (s->fmg_capped) (void)hipFree(s->fmg_capped);
    if (s->host_fmg_capped) (void)hipHostFree(s->host_fmg_capped);
    if (s->part) (void)hipFree(s->part);
    if (s->dev_scal) (void)hipFree(s->dev_scal);
    if (s->gs_state) (void)hipFree(s->gs_state);
    if (s->host_scal) (void)hipHostFree(s->host_scal);
    if (s->host_state) (void)hipHostFree(s->host_state);
    if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
    if (s->ev_end) (void)hipEventDestroy(s->ev_end);
    if (s->ev_norm) (void)hipEventDestroy(s->ev_norm);
    delete s;
}

template <typename T>
bool dev_alloc(T **p, size_t n)
{
    return MG_HIP(hipMalloc((void **)p, n * sizeof(T)));
}

// mg_cubic_table(N_src -> N_dst) in device memory; false when it does not fit prolong_cubic's tiling (needed: the
// prolongation tables) or on a HIP error
bool make_cubic_table(int N_src, int N_dst, bool for_prolongation, k::CubicTable *t)
{
    std::vector<int> base((size_t)N_dst);
    std::vector<double> w(4 * (size_t)N_dst);
    build_cubic_table(N_src, N_dst, base.data(), w.data());
    if (for_prolongation && !k::cubic_table_fits(N_src, N_dst, base.data())) {
        fail(MG_ERR_UNSUPPORTED, "cubic prolongation %d -> %d: the source windows do not fit the kernel's tiles", N_src, N_dst);
        return false;
    }
    t->N_src = N_src;
    t->N_dst = N_dst;
    return dev_alloc(&t->base, base.size()) && dev_alloc(&t->w, w.size()) &&
           MG_HIP(hipMemcpy(t->base, base.data(), base.size() * sizeof(int), hipMemcpyHostToDevice)) &&
           MG_HIP(hipMemcpy(t->w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
}

}  // namespace

// ------------------------------------------------------------------ the operator of a hierarchy (mg_internal.h: SolveOperator)
void mg::SolveOperator::sweep(hipStream_t st, int l, const double *in, const double *F, double *out) const
{
    const int N = (*sizes)[l];
    const LevelConsts &c = (*lc)[l];
    if (kind) k::wjacobi_bc(st, N, c.dx2, c.sd, o->omega, kind, a(l), in, F, out);
    else if (react) k::wjacobi_rx(st, N, c.dx2, c.sd, o->omega, a(l), s(l), in, F, out);
    else if (coef) k::wjacobi_vc(st, N, c.dx2, c.sd, o->omega, a(l), in, F, out);
    else k::wjacobi(st, N, c.dx2, c.c, in, F, out, c.sh);
}

void mg::SolveOperator::residual(hipStream_t st, int l, const double *U, const double *F, double *D) const
{
    const int N = (*sizes)[l];
    const LevelConsts &c = (*lc)[l];
    if (kind) k::residual_bc(st, N, c.inv, c.sd, kind, a(l), U, F, D, -1);
    else if (react) k::residual_rx(st, N, c.dx2, c.inv, c.sd, a(l), s(l), U, F, D, -1);
    else if (coef) k::residual_vc(st, N, c.inv, c.sd, a(l), U, F, D, -1);
    else k::residual(st, N, c.inv, U, F, D, -1, c.sh);
}

void mg::SolveOperator::restrict_residual(hipStream_t st, int l, const double *D, double *Fc) const
{
    const int N = (*sizes)[l], M = (*sizes)[l + 1];
    if (kind) k::restrict_bc(st, N, kind, D, M, Fc, restrict_table(N, M));
    else k::restrict_gather(st, N, D, M, Fc, restrict_table(N, M), +1);
}

void mg::SolveOperator::coarse_solve(hipStream_t st, double *U, const double *F, int *gs_state, double *gs_err) const
{
    const int last = (int)sizes->size() - 1, N = (*sizes)[last];
    const LevelConsts &c = (*lc)[last];
    if (kind && project_coarse)   // (four Neumann sides at shift == 0: c.sd == 0)
        k::gauss_seidel_relative_bc_mean(st, N, c.dx2, c.inv, kind, a(last), U, F, o->coarse_atol, o->coarse_rtol, o->coarse_max_iters,
                                         gs_state, gs_err, nullptr);
    else if (kind)
        k::gauss_seidel_relative_bc(st, N, c.dx2, c.inv, c.sd, kind, a(last), U, F, o->coarse_atol, o->coarse_rtol, o->coarse_max_iters,
                                    gs_state, gs_err);
    else if (react)
        k::gauss_seidel_relative_rx(st, N, c.dx2, c.inv, c.sd, a(last), s(last), U, F, o->coarse_atol, o->coarse_rtol,
                                    o->coarse_max_iters, gs_state, gs_err);
    else if (coef)
        k::gauss_seidel_relative_vc(st, N, c.dx2, c.inv, c.sd, a(last), U, F, o->coarse_atol, o->coarse_rtol, o->coarse_max_iters,
                                    gs_state, gs_err);
    else k::gauss_seidel_relative(st, N, c.dx2, c.inv, U, F, o->coarse_atol, o->coarse_rtol, o->coarse_max_iters, gs_state, gs_err, c.sh);
}

void mg::SolveOperator::prolong_add(hipStream_t st, int l, const double *Uc, const double *Uin, double *Uout) const
{
    const int N = (*sizes)[l], M = (*sizes)[l + 1];
    if (kind) k::prolong_add_bc(st, M, kind, Uc, N, Uin, Uout, (*p_lo)[l], (*p_w)[l]);
    else k::prolong(st, M, Uc, N, Uin, Uout, prolong_table(M, N));
}

void mg::SolveOperator::norm(hipStream_t st, const double *U, const double *F, double *part, double *out) const
{
    const int N = (*sizes)[0];
    const LevelConsts &c = (*lc)[0];
    if (kind) k::resnorm_bc(st, N, c.inv, c.sd, kind, a(0), U, F, part, out);   // both norms run over the unknowns
    else if (react && U) k::resnorm_rx(st, N, c.dx2, c.inv, c.sd, a(0), s(0), U, F, part, out);
    else if (coef && U) k::resnorm_vc(st, N, c.inv, c.sd, a(0), U, F, part, out);
    else k::resnorm(st, N, c.inv, U, F, part, out, c.sh);   // (the reference norm ||F|| has no operator in it)
}

void mg::SolveOperator::apply(hipStream_t st, const double *U, double *out) const
{
    const LevelConsts &c = (*lc)[0];
    if (react) k::apply_rx(st, (*sizes)[0], c.dx2, c.inv, c.sd, a(0), s(0), U, out);
    else k::apply_vc(st, (*sizes)[0], c.inv, c.sd, a(0), U, out);
}

// ------------------------------------------------------------------ the recorded cycle (mg_internal.h: SolveCycle)
SolveCycle mg::build_solve_cycle(int nl, int pre, int post, int top, bool fused, const int *down_fused, const int *up_fused, bool with_coef)
{
    SolveCycle c;
    const int last = nl - 1;
    const FieldRef none{}, U0{Field::U0, top}, F0{Field::F0, top};
    auto A = [](int l) { return FieldRef{Field::A, l}; };
    auto B = [](int l) { return FieldRef{Field::B, l}; };
    auto F = [&](int l) { return l == top ? F0 : FieldRef{Field::F, l}; };
    auto a = [&](int l) { return with_coef && !fused ? FieldRef{Field::Coef, l} : none; };
    auto emit = [&](SolveStep s) {
        for (const SolveStep &t : c.steps)
            if (t.in == s.in && t.F == s.F && t.coarse == s.coarse && t.out == s.out && t.Fc == s.Fc) s.slot = t.slot;
        if (s.slot == 0) s.slot = ++c.n_slots;
        c.steps.push_back(s);
    };
    auto node = [&](int l, int steps, int d_sign, bool transfer, FieldRef in, FieldRef coarse, FieldRef out, FieldRef Fc) {
        emit({.kind = SolveStep::Node, .level = l, .steps = steps, .d_sign = d_sign, .fused_transfer = transfer, .in = in, .F = F(l),
              .coarse = coarse, .out = out, .Fc = Fc});
    };
    auto sweep = [&](int l, FieldRef in, FieldRef out) {
        emit({.kind = SolveStep::Sweep, .level = l, .in = in, .F = F(l), .coarse = a(l), .out = out});
    };
    std::vector<FieldRef> x(nl), y(nl);   // per level: the field holding the current iterate, and the free one
    for (int l = top; l < last; ++l) {
        if (fused) {
            // level `top`: the node reads U0 and stores into B; U0 is free until the way up writes the result there
            x[l] = l == top ? B(l) : A(l);
            y[l] = l == top ? U0 : B(l);
            node(l, pre, -1, down_fused[l], l == top ? U0 : none, none, x[l], down_fused[l] ? FieldRef{Field::F, l + 1} : none);
            if (down_fused[l]) continue;
        } else {
            FieldRef cur = l == top ? U0 : A(l), other = B(l);
            int sweeps = pre;
            if (l > top) {   // memset(U, 0) (:256) folded into the first sweep
                sweep(l, none, cur);
                --sweeps;
            }
            for (int i = 0; i < sweeps; ++i) {
                sweep(l, cur, other);
                std::swap(cur, other);
            }
            x[l] = cur;
            y[l] = other;
        }
        // D = -getResidual(U) (:268, :277-280) into the free field, F_c = doRestriction(D) (:287)
        emit({.kind = SolveStep::Residual, .level = l, .in = x[l], .F = F(l), .coarse = a(l), .out = y[l]});
        emit({.kind = SolveStep::Restrict, .level = l, .in = y[l], .out = {Field::F, l + 1}});
    }
    emit({.kind = SolveStep::Coarse, .level = last, .F = {Field::F, last}, .coarse = a(last), .out = A(last)});
    x[last] = A(last);
    for (int l = last - 1; l >= top; --l) {
        if (fused && up_fused[l]) {
            const FieldRef out = l == top ? U0 : B(l);
            node(l, post, +1, true, x[l], x[l + 1], out, none);
            x[l] = out;
            continue;
        }
        // U = U + doProlongation(U_c) (:354, :368) into the free field
        FieldRef cur = x[l], other = fused ? (l == top ? U0 : B(l)) : y[l];
        emit({.kind = SolveStep::ProlongAdd, .level = l, .in = cur, .coarse = x[l + 1], .out = other});
        std::swap(cur, other);
        if (fused) {   // the sweeps back into the field the prolongation read
            node(l, post, +1, false, cur, none, other, none);
            std::swap(cur, other);
        } else {
            for (int i = 0; i < post; ++i) {
                sweep(l, cur, other);
                std::swap(cur, other);
            }
        }
        x[l] = cur;
    }
    if (!(x[top] == U0)) emit({.kind = SolveStep::Copy, .level = top, .in = x[top], .out = U0});
    return c;
}

void mg::solve_fusable_levels(const std::vector<int> &sizes, std::vector<int> *down_fused, std::vector<int> *up_fused)
{
    for (size_t l = 0; l + 1 < sizes.size(); ++l) {
        const int N = sizes[l], M = sizes[l + 1];
        down_fused->push_back(k::stream_fusable(N) && restrict_table(N, M).fusable);
        up_fused->push_back(k::stream_fusable(N) && prolong_table(M, N).fusable);
    }
}

k::SmoothNode<double> mg::solve_cycle_node(const SolveStep &s, const std::vector<int> &sizes, const std::vector<LevelConsts> &lc,
                                           const NodeBatchItem &it)
{
    const int l = s.level, N = sizes[l], M = sizes[l + 1];
    k::SmoothNode<double> nd{.N = N, .dx2 = lc[l].dx2, .inv = lc[l].inv, .in = (const double *)it.in, .F = (const double *)it.F,
                             .out = (double *)it.out, .steps = s.steps, .d_sign = s.d_sign, .cw = lc[l].c, .dc = lc[l].d,
                             .shifted = lc[l].sh.on};
    if (s.fused_transfer && s.d_sign < 0) {
        nd.Fc = (double *)it.Fc;
        nd.M = M;
        nd.rt = &restrict_table(N, M);
    } else if (s.fused_transfer) {
        nd.coarse = (const double *)it.coarse;
        nd.Nc = M;
        nd.pt = &prolong_table(M, N);
    }
    return nd;
}

int mg::run_solve_cycle(hipStream_t st, const SolveCycle &c, const SolveLevels &lv, const SolveOperator &op, const double *F0, double *U0)
{
    auto at = [&](FieldRef r) -> double * {
        switch (r.f) {
        case Field::U0: return U0;
        case Field::F0: return const_cast<double *>(F0);
        case Field::A: return (*lv.A)[r.level];
        case Field::B: return (*lv.B)[r.level];
        case Field::F: return (*lv.F)[r.level];
        case Field::Coef: return const_cast<double *>(op.a(r.level));
        case Field::None: break;
        }
        return nullptr;
    };
    int launches = 0;
    for (const SolveStep &s : c.steps) {
        const int l = s.level;
        double *in = at(s.in), *F = at(s.F), *coarse = at(s.coarse), *out = at(s.out);
        ++launches;
        switch (s.kind) {
        case SolveStep::Node: k::jacobi_stream(st, solve_cycle_node(s, *op.sizes, *op.lc, {in, F, coarse, out, at(s.Fc)})); break;
        case SolveStep::Sweep: op.sweep(st, l, in, F, out); break;
        case SolveStep::Residual: op.residual(st, l, in, F, out); break;
        case SolveStep::Restrict: op.restrict_residual(st, l, in, out); break;
        case SolveStep::Coarse: op.coarse_solve(st, out, F, lv.gs_state, lv.gs_err); break;
        case SolveStep::ProlongAdd: op.prolong_add(st, l, coarse, in, out); break;
        case SolveStep::Copy: {
            const size_t n = (size_t)(*op.sizes)[l] * (*op.sizes)[l];
            (void)MG_HIP(hipMemcpyAsync(out, in, n * sizeof(double), hipMemcpyDeviceToDevice, st));
            --launches;   // (no kernel)
            break;
        }
        }
    }
    return launches;
}

const double *mg::solver_coefficient(const mg_solver *s) { return s ? s->op.a(0) : nullptr; }
const int *mg::solver_boundary(const mg_solver *s) { return s ? s->op.kind : nullptr; }
int mg::solver_size(const mg_solver *s, double *L)
{
    if (L) *L = s->L;
    return s->N;
}

namespace {

// one cycle from level `top`: through the fused nodes of the streaming smoother (its weighted instantiations), which are the
// constant operator's -- a boundary kind, a coefficient or a reaction goes operator by operator whatever mg_set_smoother says
// (top == 0 with any of them: the full-multigrid start excludes all three)
void vcycle(mg_solver *s, hipStream_t st, const double *F0, double *U0, int top = 0)
{
    const bool fused = !(s->op.kind || s->op.coef || s->op.react || ctx().smoother == SMOOTHER_SIMPLE);
    (void)run_solve_cycle(st, s->cyc[fused][top], s->lv, s->op, F0, U0);
}

// The full-multigrid start (include/mg_hip.h, mg_solve_opts.fmg): the interior of U0 becomes the FMG guess, its rim is
// read only.  u_l lives in A[l] (the caller's U at l = 0), which a cycle started at level l treats as a solve treats the
// caller's U; A[l+1], B[l+1] and F[l+1] are free again by then (u_{l+1} has been interpolated).  Launches: nl-1 restrictions,
// 1 + (nl-1) rim launches, 5 for the coarsest level, then per level the prolongation, and below level 0 the rim, fmg cycles
// started there and the cap flag.
void fmg_start(mg_solver *s, hipStream_t st, const double *F0, double *U0)
{
    const mg_solve_opts &o = s->o;
    const int nl = (int)s->sizes.size(), last = nl - 1;
    const std::vector<LevelConsts> &lc = s->lc;
    (void)MG_HIP(hipMemsetAsync(s->fmg_capped, 0, sizeof(int), st));
    for (int l = 0; l < last; ++l)
        k::restrict_gather(st, s->sizes[l], l == 0 ? F0 : s->FF[l], s->sizes[l + 1], s->FF[l + 1],
                           restrict_table(s->sizes[l], s->sizes[l + 1]), +1);
    k::rim_extract(st, s->N, U0, s->G[0]);
    for (int l = 0; l < last; ++l) k::rim_sample(st, s->down[l], s->G[l], s->G[l + 1]);
    const int Nc = s->sizes[last];
    k::rim_fill(st, Nc, s->G[last], s->B[last], true);
    k::residual(st, Nc, lc[last].inv, s->B[last], s->FF[last], s->F[last], -1, lc[last].sh);
    k::gauss_seidel_relative(st, Nc, lc[last].dx2, lc[last].inv, s->A[last], s->F[last], o.coarse_atol, o.coarse_rtol,
                             o.coarse_max_iters, s->gs_state, s->dev_scal + 2, lc[last].sh);
    k::rim_fill(st, Nc, s->G[last], s->A[last], false);
    k::flag_or(st, s->gs_state, s->fmg_capped);
    for (int l = last - 1; l >= 0; --l) {
        double *u = l == 0 ? U0 : s->A[l];
        k::prolong_cubic(st, s->up[l], s->A[l + 1], u);
        if (l == 0) break;
        k::rim_fill(st, s->sizes[l], s->G[l], u, false);
        for (int c = 0; c < o.fmg; ++c) {
            vcycle(s, st, s->FF[l], u, l);
            k::flag_or(st, s->gs_state, s->fmg_capped);
        }
    }
    (void)MG_HIP(hipMemcpyAsync(s->host_fmg_capped, s->fmg_capped, sizeof(int), hipMemcpyDeviceToHost, st));
}

// enqueue ||F - AU|| (U == nullptr: ||F||) into dev_scal[slot]
void norm(mg_solver *s, hipStream_t st, const double *F0, const double *U0, int slot)
{
    // (timed for scripts/bench_solve_singular.py, the yardstick of the weighted sum: U, F and, with one, the coefficient)
    ProfScope ps(U0 ? "resnorm" : "refnorm", s->N, (double)s->N * s->N * (U0 ? 16.0 + (s->op.coef ? 8.0 : 0.0) + (s->op.react ? 8.0 : 0.0) : 8.0), st);
    s->op.norm(st, U0, F0, s->part, s->dev_scal + slot);
}

bool read_back(mg_solver *s, hipStream_t st)
{
    if (!MG_HIP(hipMemcpyAsync(s->host_scal, s->dev_scal, 4 * sizeof(double), hipMemcpyDeviceToHost, st))) return false;
    if (!MG_HIP(hipMemcpyAsync(s->host_state, s->gs_state, 4 * sizeof(int), hipMemcpyDeviceToHost, st))) return false;
    if (!MG_HIP(hipEventRecord(s->ev_norm, st))) return false;
    return MG_HIP(hipEventSynchronize(s->ev_norm));
}

// ------------------------------------------------------------------ Krylov acceleration (include/mg_krylov.h)
constexpr int KR_B = 0, KR_W = MG_KRYLOV_MAX_M, KR_ALPHA = 2 * MG_KRYLOV_MAX_M, KR_RHO = KR_ALPHA + 1, KR_BRK = KR_ALPHA + 2,
              KR_SCALARS = KR_ALPHA + 3;
constexpr int KR_REC_MAX = MG_KRYLOV_MAX_M + 7;

// r = -(inv*b(U) - F): the launch of the cycle's signed residual at level 0
void krylov_residual(mg_solver *s, hipStream_t st, const double *F0, const double *U0) { s->op.residual(st, 0, U0, F0, s->kr_r); }

// the read-back of an iteration: rho_rec and the breakdown flag, the coarse solve's state and (with_norm: a restart) dev_scal
bool krylov_read_back(mg_solver *s, hipStream_t st, bool with_norm)
{
    if (!MG_HIP(hipMemcpyAsync(s->kr_host, s->kr_scal + KR_RHO, 2 * sizeof(double), hipMemcpyDeviceToHost, st))) return false;
    if (with_norm) return read_back(s, st);
    if (!MG_HIP(hipMemcpyAsync(s->host_state, s->gs_state, 4 * sizeof(int), hipMemcpyDeviceToHost, st))) return false;
    if (!MG_HIP(hipEventRecord(s->ev_norm, st))) return false;
    return MG_HIP(hipEventSynchronize(s->ev_norm));
}

// the loop of include/mg_krylov.h from history[0] = *res on; false on a HIP error
bool krylov_iterate(mg_solver *s, hipStream_t st, const double *F0, double *U0, double tol, mg_solve_result *r, double *res)
{
    const mg_solve_opts &o = s->o;
    const int N = s->N, m = s->kr_m, rec_len = m + 7;
    const size_t n = (size_t)N * N;
    const double pts = (double)N * N;
    s->kr_log_m = m;
    s->kr_records = 0;
    s->kr_breakdown = false;
    int kk = 0;
    if (!(*res <= tol) && r->cycles < o.max_cycles) krylov_residual(s, st, F0, U0);
    while (!(*res <= tol) && r->cycles < o.max_cycles) {
        double *z = s->kr_Z[kk], *q = s->kr_Q[kk];
        double *rec = s->kr_log + (size_t)r->cycles * rec_len;
        k::KrylovVecs v{};
        for (int j = 0; j < kk; ++j) {
            v.q[j] = s->kr_Q[j];
            v.z[j] = s->kr_Z[j];
        }
        if (!MG_HIP(hipMemsetAsync(z, 0, n * sizeof(double), st))) return false;
        vcycle(s, st, s->kr_r, z);
        s->op.apply(st, z, q);
        if (kk > 0) {
            ProfScope ps("krylov_dots", N, pts * (8.0 + 8.0 * kk));
            k::krylov_dots(st, N, kk, q, v, s->kr_part, s->kr_scal + KR_W, s->kr_scal + KR_B, rec + 1);
        }
        {
            ProfScope ps("krylov_orth", N, pts * (kk > 0 ? 40.0 + 16.0 * kk : 16.0));
            k::krylov_orth(st, N, kk, q, z, s->kr_r, v, s->kr_scal + KR_B, s->kr_part);
        }
        k::krylov_orth_finish(st, N, s->kr_part, kk, m, rec + 1 + m, s->kr_scal + KR_W + kk, s->kr_scal + KR_ALPHA, s->kr_scal + KR_BRK,
                              rec);
        {
            ProfScope ps("krylov_update", N, pts * 48.0);
            k::krylov_update(st, N, s->kr_scal + KR_ALPHA, U0, z, s->kr_r, q, s->kr_part);
        }
        k::krylov_update_finish(st, N, s->kr_part, nullptr, s->kr_scal + KR_RHO, rec + m + 4);
        r->cycles += 1;
        kk += 1;
        bool restart = kk == m;   // (known here: the recomputation is enqueued behind the update and read with it)
        if (!restart) {
            if (!krylov_read_back(s, st, false)) return false;
            *res = s->kr_host[0];
            restart = *res <= tol;
        }
        if (restart) {
            krylov_residual(s, st, F0, U0);
            norm(s, st, F0, U0, 0);
            k::krylov_log_restart(st, rec + m + 4, s->dev_scal);
            if (!krylov_read_back(s, st, true)) return false;
            *res = s->host_scal[0];
            kk = 0;
        }
        s->history.push_back(*res);
        s->kr_records = r->cycles;
        if (s->host_state[2]) r->coarse_capped = 1;
        if (s->kr_host[1] != 0.0) {
            s->kr_breakdown = true;
            break;
        }
    }
    if (s->kr_records > 0 &&
        !MG_HIP(hipMemcpyAsync(s->kr_log_host.data(), s->kr_log, (size_t)s->kr_records * rec_len * sizeof(double), hipMemcpyDeviceToHost, st)))
        return false;
    return true;
}

}  // namespace

bool mg::solve_opts_ok(const char *who, int N, double L, const mg_solve_opts &o) { return opts_ok(who, N, L, o); }

std::vector<LevelConsts> mg::solve_level_consts(const std::vector<int> &sizes, double L, const mg_solve_opts &o)
{
    std::vector<LevelConsts> lc;
    for (int N : sizes) {
        LevelConsts c;
        c.dx2 = spacing_sq(N, L);
        c.inv = 1.0 / c.dx2;
        c.sd = o.shift * c.dx2;
        c.d = 4.0 + c.sd;
        c.q = 1.0 / c.d;
        c.c = o.omega * c.q;
        c.sh = k::Shifted{o.shift != 0.0, c.d, c.q};
        lc.push_back(c);
    }
    return lc;
}

extern "C" {

void mg_solve_opts_default(mg_solve_opts *o)
{
    if (!o) return;
    o->pre = 3;
    o->post = 3;
    o->N_min = 8;
    o->omega = 0.8;
    o->coarse_rtol = 1e-2;
    o->coarse_atol = 0.0;
    o->coarse_max_iters = 10000;
    o->rtol = 1e-10;
    o->atol = 0.0;
    o->max_cycles = 50;
    o->shift = 0.0;
    o->fmg = 0;
}

int mg_solve_cycle_describe(int nl, int pre, int post, int top, int fused, const int *down_fused, const int *up_fused, int with_coef,
                            int *out, int cap)
{
    if (nl < 2 || pre < 1 || post < 1 || top < 0 || top > nl - 2 || (fused && (!down_fused || !up_fused))) {
        fail(MG_ERR_ARG, "mg_solve_cycle_describe: nl = %d (at least 2), pre = %d, post = %d (at least 1 each), top = %d (inside "
                         "[0, nl - 2]), or a fused cycle without its fusable levels", nl, pre, post, top);
        return -1;
    }
    const SolveCycle c = build_solve_cycle(nl, pre, post, top, fused != 0, down_fused, up_fused, with_coef != 0);
    const int n = (int)c.steps.size();
    for (int i = 0; out && i < n && i < cap; ++i) {
        const SolveStep &s = c.steps[i];
        int *r = out + (size_t)i * MG_SOLVE_CYCLE_RECORD;
        *r++ = s.kind;
        *r++ = s.level;
        *r++ = s.steps;
        *r++ = s.d_sign;
        *r++ = s.fused_transfer;
        for (const FieldRef &f : {s.in, s.F, s.coarse, s.out, s.Fc}) {
            *r++ = (int)f.f;
            *r++ = f.level;
        }
        *r = s.slot;
    }
    return n;
}

mg_solver *mg_solver_create(int N, double L, const mg_solve_opts *opts)
{
    if (!require_ready("mg_solver_create")) return nullptr;
    mg_solve_opts o;
    mg_solve_opts_default(&o);
    if (opts) o = *opts;
    if (!solve_opts_ok("mg_solver_create", N, L, o)) return nullptr;
    mg_solver *s = new mg_solver;
    s->N = N;
    s->L = L;
    s->o = o;
    for (int n = N; n >= o.N_min; n /= 2) s->sizes.push_back(n);   // mg_cycle_load's halving sizes (con_N = 1)
    const int nl = (int)s->sizes.size();
    s->lc = solve_level_consts(s->sizes, L, o);
    s->op = SolveOperator{&s->o, &s->sizes, &s->lc, nullptr, nullptr, &s->bc_lo, &s->bc_w};
    if (!k::gs_relative_fits(s->sizes[nl - 1])) {   // (N_min <= 32 keeps the coarsest level below 64)
        fail(MG_ERR_UNSUPPORTED, "mg_solver_create: coarsest level %d does not fit the coarse solver", s->sizes[nl - 1]);
        release(s);
        return nullptr;
    }
    s->A.assign(nl, nullptr);
    s->B.assign(nl, nullptr);
    s->F.assign(nl, nullptr);
    bool ok = true;
    for (int l = 0; l < nl && ok; ++l) {
        const size_t n = (size_t)s->sizes[l] * s->sizes[l];
        ok = dev_alloc(&s->B[l], n);
        if (ok && l > 0) ok = dev_alloc(&s->A[l], n) && dev_alloc(&s->F[l], n);
        if (ok && pool_poison_wanted())   // MG_POOL_POISON: no level array starts from what hipMalloc happened to return
            for (double *a : {s->A[l], s->B[l], s->F[l]}) poison_block(a, n * sizeof(double));
    }
    for (int l = 0; l + 1 < nl && ok; ++l) {   // the transfer tables, built once here
        const int Nf = s->sizes[l], Nc = s->sizes[l + 1];
        ok = restrict_table(Nf, Nc).lo != nullptr && prolong_table(Nc, Nf).owner_row != nullptr;
    }
    ok = ok && dev_alloc(&s->part, k::resnorm_partials(N)) && dev_alloc(&s->dev_scal, 4) && dev_alloc(&s->gs_state, 4) &&
         MG_HIP(hipHostMalloc((void **)&s->host_scal, 4 * sizeof(double), hipHostMallocDefault)) &&
         MG_HIP(hipHostMalloc((void **)&s->host_state, 4 * sizeof(int), hipHostMallocDefault)) &&
         MG_HIP(hipEventCreate(&s->ev_begin)) && MG_HIP(hipEventCreate(&s->ev_end)) &&
         MG_HIP(hipEventCreateWithFlags(&s->ev_norm, hipEventDisableTiming));
    if (ok && pool_poison_wanted()) poison_block(s->part, k::resnorm_partials(N) * sizeof(double));
    if (ok && o.fmg >= 1) {   // the arrays and tables of the full-multigrid start
        s->FF.assign(nl, nullptr);
        s->G.assign(nl, nullptr);
        s->up.resize(nl - 1);
        s->down.resize(nl - 1);
        for (int l = 0; l < nl && ok; ++l) {
            const size_t n = (size_t)s->sizes[l] * s->sizes[l];
            ok = dev_alloc(&s->G[l], 4 * (size_t)s->sizes[l]);
            if (ok && l > 0) ok = dev_alloc(&s->FF[l], n);
            if (ok && pool_poison_wanted()) {
                poison_block(s->G[l], 4 * (size_t)s->sizes[l] * sizeof(double));
                poison_block(s->FF[l], n * sizeof(double));
            }
        }
        for (int l = 0; l + 1 < nl && ok; ++l)
            ok = make_cubic_table(s->sizes[l + 1], s->sizes[l], true, &s->up[l]) &&
                 make_cubic_table(s->sizes[l], s->sizes[l + 1], false, &s->down[l]);
        ok = ok && dev_alloc(&s->fmg_capped, 1) &&
             MG_HIP(hipHostMalloc((void **)&s->host_fmg_capped, sizeof(int), hipHostMallocDefault));
        if (ok) *s->host_fmg_capped = 0;
    }
    ok = ok && MG_HIP(hipStreamSynchronize(ctx().stream));   // (the fills ran on the engine's stream; a solve may run on another)
    ok = ok && MG_HIP(hipMemset(s->dev_scal, 0, 4 * sizeof(double))) && MG_HIP(hipMemset(s->gs_state, 0, 4 * sizeof(int)));
    if (!ok) {
        release(s);
        return nullptr;
    }
    s->lv = SolveLevels{&s->A, &s->B, &s->F, s->gs_state, s->dev_scal + 2};
    std::vector<int> down_fused, up_fused;
    solve_fusable_levels(s->sizes, &down_fused, &up_fused);
    for (int top = 0; top < (o.fmg >= 1 ? nl - 1 : 1); ++top)
        for (int fused = 0; fused < 2; ++fused)
            s->cyc[fused].push_back(build_solve_cycle(nl, o.pre, o.post, top, fused, down_fused.data(), up_fused.data(), false));
    s->history.reserve((size_t)o.max_cycles + 1);
    return s;
}

int mg_solver_solve(mg_solver *s, const double *F_dev, double *U_dev, mg_solve_result *out)
{
    mg_solve_result r;
    std::memset(&r, 0, sizeof r);
    auto finish = [&](int status) {
        r.status = status;
        r.n_history = (int)(s ? s->history.size() : 0);
        r.history = s && !s->history.empty() ? s->history.data() : nullptr;
        if (out) *out = r;
        return status;
    };
    if (!require_ready("mg_solver_solve")) return finish(MG_ERR_NOT_INIT);
    if (!s || !F_dev || !U_dev) {
        fail(MG_ERR_ARG, "mg_solver_solve: NULL solver or array");
        return finish(MG_ERR_ARG);
    }
    if (((uintptr_t)F_dev | (uintptr_t)U_dev) % 16 != 0) {
        fail(MG_ERR_ARG, "mg_solver_solve: F and U must be 16-byte aligned");
        return finish(MG_ERR_ARG);
    }
    s->history.clear();
    const hipStream_t st = ctx().stream;
    const mg_solve_opts &o = s->o;
    if (!MG_HIP(hipEventRecord(s->ev_begin, st))) return finish(MG_ERR_HIP);
    if (!MG_HIP(hipMemsetAsync(s->gs_state, 0, 4 * sizeof(int), st))) return finish(MG_ERR_HIP);
    // the singular problem (include/mg_singular.h): everything below works on Ft = F - mean_w(F) in the solver's own buffer
    const bool singular = s->op.kind && s->op.project_coarse;
    s->sing_info[0] = s->sing_info[1] = s->sing_info[2] = 0.0;
    if (singular) {
        k::weighted_mean(st, s->N, F_dev, 0.0, s->part, s->sing_scal);
        k::shift_by(st, s->N, F_dev, s->sing_scal + 1, s->sing_F);
        F_dev = s->sing_F;
    }
    norm(s, st, F_dev, nullptr, 1);
    norm(s, st, F_dev, U_dev, 0);
    if (!read_back(s, st)) return finish(MG_ERR_HIP);
    r.ref_norm = s->host_scal[1];
    double res = s->host_scal[0];
    r.res0 = res;
    s->history.push_back(res);
    const double tol = std::fmax(o.rtol * r.ref_norm, o.atol);
    const bool fmg = o.fmg >= 1 && !(res <= tol);
    const bool krylov = s->kr_m > 0;   // (fmg == 0 with it: mg_solver_set_krylov refuses the combination)
    if (krylov && !krylov_iterate(s, st, F_dev, U_dev, tol, &r, &res)) return finish(MG_ERR_HIP);
    if (fmg) {
        fmg_start(s, st, F_dev, U_dev);
        if (o.max_cycles == 0 && !read_back(s, st)) return finish(MG_ERR_HIP);   // (the loop's read-back otherwise)
    }
    while (!krylov && !(res <= tol) && r.cycles < o.max_cycles) {
        vcycle(s, st, F_dev, U_dev);
        norm(s, st, F_dev, U_dev, 0);
        if (!read_back(s, st)) return finish(MG_ERR_HIP);
        res = s->host_scal[0];
        s->history.push_back(res);
        r.cycles += 1;
        if (s->host_state[2]) r.coarse_capped = 1;
    }
    if (singular) {   // the gauge, after the last cycle: U <- U - (mean_w(U) - mean), the constant staying on the device
        k::weighted_mean(st, s->N, U_dev, s->mean, s->part, s->sing_scal + 2);
        k::shift_by(st, s->N, U_dev, s->sing_scal + 3, U_dev);
        if (!MG_HIP(hipMemcpyAsync(s->sing_host, s->sing_scal, 4 * sizeof(double), hipMemcpyDeviceToHost, st))) return finish(MG_ERR_HIP);
    }
    if (!MG_HIP(hipEventRecord(s->ev_end, st)) || !MG_HIP(hipEventSynchronize(s->ev_end))) return finish(MG_ERR_HIP);
    float ms = 0.0f;
    if (MG_HIP(hipEventElapsedTime(&ms, s->ev_begin, s->ev_end))) r.device_ms = ms;
    if (fmg && *s->host_fmg_capped) r.coarse_capped = 1;
    if (singular) {   // (the copy was enqueued before ev_end, which has been waited for)
        s->sing_info[0] = s->sing_host[0];
        s->sing_info[1] = s->sing_host[2];
        s->sing_info[2] = s->mean;
    }
    r.res = res;
    r.converged = res <= tol ? 1 : 0;
    return finish(r.converged ? MG_SOLVE_CONVERGED : MG_SOLVE_NOT_CONVERGED);
}

void mg_prolongCubic(int N_src, const double *U_c, int N_dst, double *U_f)
{
    if (!require_ready("mg_prolongCubic")) return;
    if (N_src < 3 || N_dst < 3 || !U_c || !U_f) {
        fail(MG_ERR_ARG, "mg_prolongCubic: N_src = %d, N_dst = %d (at least 3 each) or a NULL array", N_src, N_dst);
        return;
    }
    if (((uintptr_t)U_c | (uintptr_t)U_f) % 16 != 0) {
        fail(MG_ERR_ARG, "mg_prolongCubic: U_c and U_f must be 16-byte aligned");
        return;
    }
    // (the solver keeps its tables from creation on; this entry point builds the one it needs and lets go of it)
    k::CubicTable t;
    if (make_cubic_table(N_src, N_dst, true, &t)) {
        k::prolong_cubic(ctx().stream, t, U_c, U_f);
        (void)MG_HIP(hipStreamSynchronize(ctx().stream));
    }
    if (t.base) (void)hipFree(t.base);
    if (t.w) (void)hipFree(t.w);
}

// ------------------------------------------------------------------ variable coefficient (include/mg_varcoef.h)
int mg_solver_set_coefficient(mg_solver *s, const double *a_dev)
{
    if (!require_ready("mg_solver_set_coefficient")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_solver_set_coefficient: NULL solver");
        return MG_ERR_ARG;
    }
    if (!a_dev) {   // back to the constant-coefficient solver (the level storage stays for the next coefficient)
        s->op.coef = nullptr;
        return MG_OK;
    }
    if (s->o.fmg != 0) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_coefficient: the solver was created with fmg = %d; the full-multigrid start is not "
                                 "built for a variable coefficient", s->o.fmg);
        return MG_ERR_UNSUPPORTED;
    }
    if ((uintptr_t)a_dev % 16 != 0) {
        fail(MG_ERR_ARG, "mg_solver_set_coefficient: a must be 16-byte aligned");
        return MG_ERR_ARG;
    }
    const hipStream_t st = ctx().stream;
    const int nl = (int)s->sizes.size();
    if (s->coef.empty()) {   // the first coefficient: level storage, about 4/3 N^2 doubles
        s->coef.assign(nl, nullptr);
        bool ok = dev_alloc(&s->coef_flag, 1) && MG_HIP(hipHostMalloc((void **)&s->host_coef_flag, sizeof(int), hipHostMallocDefault));
        for (int l = 0; l < nl && ok; ++l) ok = dev_alloc(&s->coef[l], (size_t)s->sizes[l] * s->sizes[l]);
        if (!ok) {   // (release() frees what was allocated; the next call starts over)
            for (double *&p : s->coef) if (p) { (void)hipFree(p); p = nullptr; }
            s->coef.clear();
            if (s->coef_flag) { (void)hipFree(s->coef_flag); s->coef_flag = nullptr; }
            if (s->host_coef_flag) { (void)hipHostFree(s->host_coef_flag); s->host_coef_flag = nullptr; }
            return MG_ERR_HIP;
        }
    }
    // the check comes first and reads the CALLER's array: a refused coefficient leaves the solver's own untouched
    const size_t n0 = (size_t)s->N * s->N;
    if (!MG_HIP(hipMemsetAsync(s->coef_flag, 0, sizeof(int), st))) return MG_ERR_HIP;
    k::coef_check(st, a_dev, n0, s->coef_flag);
    if (!MG_HIP(hipMemcpyAsync(s->host_coef_flag, s->coef_flag, sizeof(int), hipMemcpyDeviceToHost, st)) ||
        !MG_HIP(hipStreamSynchronize(st)))
        return MG_ERR_HIP;
    if (*s->host_coef_flag) {
        fail(MG_ERR_ARG, "mg_solver_set_coefficient: every value of a must be finite and > 0");
        return MG_ERR_ARG;
    }
    // from here on the level storage is overwritten: until it is whole again the solver has NO coefficient, so a HIP error
    // below leaves the constant-coefficient solver, never one on a half-replaced coefficient
    s->op.coef = nullptr;
    if (!MG_HIP(hipMemcpyAsync(s->coef[0], a_dev, n0 * sizeof(double), hipMemcpyDeviceToDevice, st))) return MG_ERR_HIP;
    for (int l = 0; l + 1 < nl; ++l)
        k::coef_coarsen(st, s->sizes[l], s->coef[l], s->sizes[l + 1], s->coef[l + 1], restrict_table(s->sizes[l], s->sizes[l + 1]));
    if (!MG_HIP(hipStreamSynchronize(st))) return MG_ERR_HIP;   // (the caller may free a, or solve on another stream)
    s->op.coef = &s->coef;
    return MG_OK;
}

int mg_solver_has_coefficient(const mg_solver *s) { return s && s->op.coef ? 1 : 0; }

namespace {
bool vc_args_ok(const char *who, int N, double L, double shift, std::initializer_list<const void *> arrays)
{
    if (N < 3 || !(L > 0.0) || !finite(L) || !(shift >= 0.0) || !finite(shift)) {
        fail(MG_ERR_ARG, "%s: N = %d (at least 3), L = %g (positive, finite), shift = %g (finite, >= 0)", who, N, L, shift);
        return false;
    }
    for (const void *p : arrays)
        if (!p || (uintptr_t)p % 16 != 0) {
            fail(MG_ERR_ARG, "%s: a NULL or not 16-byte aligned array", who);
            return false;
        }
    return true;
}
}  // namespace

void mg_applyOperator(int N, double L, double shift, const double *a_dev, const double *U, double *out)
{
    if (!require_ready("mg_applyOperator") || !vc_args_ok("mg_applyOperator", N, L, shift, {U, out})) return;
    if ((uintptr_t)a_dev % 16 != 0) {
        fail(MG_ERR_ARG, "mg_applyOperator: a must be 16-byte aligned");
        return;
    }
    const double dx2 = spacing_sq(N, L);
    k::apply_vc(ctx().stream, N, 1.0 / dx2, shift * dx2, a_dev, U, out);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_coarsenCoefficient(int N, const double *a_f, int M, double *a_c)
{
    if (!require_ready("mg_coarsenCoefficient")) return;
    if (N < 3 || M < 2 || !a_f || !a_c) {
        fail(MG_ERR_ARG, "mg_coarsenCoefficient: N = %d (at least 3), M = %d (at least 2) or a NULL array", N, M);
        return;
    }
    const RestrictTable &t = restrict_table(N, M);   // (refuses a table that leaves the fine grid)
    if (!t.lo) return;
    k::coef_coarsen(ctx().stream, N, a_f, M, a_c, t);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_sweepCoefficient(int N, double L, double shift, double omega, const double *a_dev, const double *U_in, const double *F,
                         double *U_out)
{
    if (!require_ready("mg_sweepCoefficient") || !vc_args_ok("mg_sweepCoefficient", N, L, shift, {a_dev, F, U_out})) return;
    if ((uintptr_t)U_in % 16 != 0 || !(omega > 0.0 && omega <= 1.0)) {
        fail(MG_ERR_ARG, "mg_sweepCoefficient: U_in must be 16-byte aligned, omega = %g inside (0, 1]", omega);
        return;
    }
    const double dx2 = spacing_sq(N, L);
    {
        ProfScope ps("wjacobi_vc", N, (double)N * N * 32.0);   // (the yardstick of scripts/bench_solve_reaction.py)
        k::wjacobi_vc(ctx().stream, N, dx2, shift * dx2, omega, a_dev, U_in, F, U_out);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_residualCoefficient(int N, double L, double shift, const double *a_dev, const double *U, const double *F, double *D, int sign)
{
    if (!require_ready("mg_residualCoefficient") || !vc_args_ok("mg_residualCoefficient", N, L, shift, {a_dev, U, F, D})) return;
    const double dx2 = spacing_sq(N, L);
    {
        ProfScope ps("residual_vc", N, (double)N * N * 32.0);   // (the yardstick of scripts/bench_heat_vc.py: the same 32 B per point)
        k::residual_vc(ctx().stream, N, 1.0 / dx2, shift * dx2, a_dev, U, F, D, sign < 0 ? -1 : +1);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

// ------------------------------------------------------------------ variable reaction term (include/mg_reaction.h)
namespace {
// the reaction's level storage, about 4/3 N^2 doubles, and the flag of its check: allocated by the first call that needs them
// (mg_solver_set_reaction, mg_solver_newton) and reused; false on a HIP error (the next call starts over)
bool react_storage(mg_solver *s)
{
    if (!s->react.empty()) return true;
    const int nl = (int)s->sizes.size();
    s->react.assign(nl, nullptr);
    bool ok = dev_alloc(&s->react_flag, 1) && MG_HIP(hipHostMalloc((void **)&s->host_react_flag, sizeof(int), hipHostMallocDefault));
    for (int l = 0; l < nl && ok; ++l) ok = dev_alloc(&s->react[l], (size_t)s->sizes[l] * s->sizes[l]);
    if (!ok) {
        for (double *&p : s->react) if (p) { (void)hipFree(p); p = nullptr; }
        s->react.clear();
        if (s->react_flag) { (void)hipFree(s->react_flag); s->react_flag = nullptr; }
        if (s->host_react_flag) { (void)hipHostFree(s->host_react_flag); s->host_react_flag = nullptr; }
    }
    return ok;
}
}  // namespace

int mg_solver_set_reaction(mg_solver *s, const double *s_dev)
{
    if (!require_ready("mg_solver_set_reaction")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_solver_set_reaction: NULL solver");
        return MG_ERR_ARG;
    }
    if (!s_dev) {   // the solver without a reaction again (the level storage stays for the next one)
        s->op.react = nullptr;
        return MG_OK;
    }
    if (s->o.fmg != 0) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_reaction: the solver was created with fmg = %d; the full-multigrid start is not "
                                 "built for a reaction term", s->o.fmg);
        return MG_ERR_UNSUPPORTED;
    }
    if (s->op.kind) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_reaction: a boundary with a Neumann side is set; a reaction together with boundary "
                                 "kinds is not built");
        return MG_ERR_UNSUPPORTED;
    }
    if ((uintptr_t)s_dev % 16 != 0) {
        fail(MG_ERR_ARG, "mg_solver_set_reaction: s must be 16-byte aligned");
        return MG_ERR_ARG;
    }
    const hipStream_t st = ctx().stream;
    const int nl = (int)s->sizes.size();
    if (!react_storage(s)) return MG_ERR_HIP;
    // the check comes first and reads the CALLER's array: a refused reaction leaves the solver's own untouched
    const size_t n0 = (size_t)s->N * s->N;
    if (!MG_HIP(hipMemsetAsync(s->react_flag, 0, sizeof(int), st))) return MG_ERR_HIP;
    k::reaction_check(st, s_dev, n0, s->react_flag);
    if (!MG_HIP(hipMemcpyAsync(s->host_react_flag, s->react_flag, sizeof(int), hipMemcpyDeviceToHost, st)) ||
        !MG_HIP(hipStreamSynchronize(st)))
        return MG_ERR_HIP;
    if (*s->host_react_flag) {
        fail(MG_ERR_ARG, "mg_solver_set_reaction: every value of s must be finite and >= 0 (a negative or not finite value found)");
        return MG_ERR_ARG;
    }
    // from here on the level storage is overwritten: until it is whole again the solver has NO reaction
    s->op.react = nullptr;
    if (!MG_HIP(hipMemcpyAsync(s->react[0], s_dev, n0 * sizeof(double), hipMemcpyDeviceToDevice, st))) return MG_ERR_HIP;
    for (int l = 0; l + 1 < nl; ++l)
        k::coef_coarsen(st, s->sizes[l], s->react[l], s->sizes[l + 1], s->react[l + 1], restrict_table(s->sizes[l], s->sizes[l + 1]));
    if (!MG_HIP(hipStreamSynchronize(st))) return MG_ERR_HIP;   // (the caller may free s, or solve on another stream)
    s->op.react = &s->react;
    return MG_OK;
}

int mg_solver_has_reaction(const mg_solver *s) { return s && s->op.react ? 1 : 0; }

namespace {
// the optional coefficient of a reaction hook: NULL, or 16-byte aligned
bool rx_coef_ok(const char *who, const double *a_dev)
{
    if ((uintptr_t)a_dev % 16 == 0) return true;
    fail(MG_ERR_ARG, "%s: a must be 16-byte aligned", who);
    return false;
}
}  // namespace

void mg_applyOperatorReaction(int N, double L, double shift, const double *a_dev, const double *s_dev, const double *U, double *out)
{
    if (!require_ready("mg_applyOperatorReaction") || !vc_args_ok("mg_applyOperatorReaction", N, L, shift, {s_dev, U, out}) ||
        !rx_coef_ok("mg_applyOperatorReaction", a_dev))
        return;
    const double dx2 = spacing_sq(N, L);
    k::apply_rx(ctx().stream, N, dx2, 1.0 / dx2, shift * dx2, a_dev, s_dev, U, out);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_sweepReaction(int N, double L, double shift, double omega, const double *a_dev, const double *s_dev, const double *U_in,
                      const double *F, double *U_out)
{
    if (!require_ready("mg_sweepReaction") || !vc_args_ok("mg_sweepReaction", N, L, shift, {s_dev, F, U_out}) ||
        !rx_coef_ok("mg_sweepReaction", a_dev))
        return;
    if ((uintptr_t)U_in % 16 != 0 || !(omega > 0.0 && omega <= 1.0)) {
        fail(MG_ERR_ARG, "mg_sweepReaction: U_in must be 16-byte aligned, omega = %g inside (0, 1]", omega);
        return;
    }
    const double dx2 = spacing_sq(N, L);
    {
        ProfScope ps(a_dev ? "wjacobi_rx_a" : "wjacobi_rx", N, (double)N * N * (a_dev ? 40.0 : 32.0));   // (scripts/bench_solve_reaction.py)
        k::wjacobi_rx(ctx().stream, N, dx2, shift * dx2, omega, a_dev, s_dev, U_in, F, U_out);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_residualReaction(int N, double L, double shift, const double *a_dev, const double *s_dev, const double *U, const double *F,
                         double *D, int sign)
{
    if (!require_ready("mg_residualReaction") || !vc_args_ok("mg_residualReaction", N, L, shift, {s_dev, U, F, D}) ||
        !rx_coef_ok("mg_residualReaction", a_dev))
        return;
    const double dx2 = spacing_sq(N, L);
    {
        ProfScope ps(a_dev ? "residual_rx_a" : "residual_rx", N, (double)N * N * (a_dev ? 40.0 : 32.0));   // (the yardstick of scripts/bench_newton.py)
        k::residual_rx(ctx().stream, N, dx2, 1.0 / dx2, shift * dx2, a_dev, s_dev, U, F, D, sign < 0 ? -1 : +1);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_coarseSolveReaction(int N, double L, double shift, const double *a_dev, const double *s_dev, const double *F, double atol,
                            double rtol, int max_iters, double *U_out)
{
    if (!require_ready("mg_coarseSolveReaction") || !vc_args_ok("mg_coarseSolveReaction", N, L, shift, {s_dev, F, U_out}) ||
        !rx_coef_ok("mg_coarseSolveReaction", a_dev))
        return;
    if (!k::gs_relative_fits(N) || !(atol >= 0.0) || !(rtol >= 0.0) || !std::isfinite(atol) || !std::isfinite(rtol) || max_iters < 1) {
        fail(MG_ERR_ARG, "mg_coarseSolveReaction: 3 <= N = %d < %d, atol, rtol >= 0 and finite, max_iters >= 1", N, k::GS_RELATIVE_MAX_N);
        return;
    }
    Context &c = ctx();
    const double dx2 = spacing_sq(N, L);
    if (!MG_HIP(hipMemsetAsync(c.gs_state, 0, 4 * sizeof(int), c.stream))) return;
    k::gauss_seidel_relative_rx(c.stream, N, dx2, 1.0 / dx2, shift * dx2, a_dev, s_dev, U_out, F, atol, rtol, max_iters, c.gs_state, nullptr);
    (void)MG_HIP(hipStreamSynchronize(c.stream));
}

// ------------------------------------------------------------------ semilinear problem (include/mg_newton.h)
namespace {
bool newton_kind_ok(const char *who, int kind, double kappa)
{
    if (kind != MG_NEWTON_CUBIC && kind != MG_NEWTON_SINH && kind != MG_NEWTON_EXP) {
        fail(MG_ERR_ARG, "%s: unknown kind %d (MG_NEWTON_CUBIC = 0, MG_NEWTON_SINH = 1, MG_NEWTON_EXP = 2)", who, kind);
        return false;
    }
    if (!(kappa >= 0.0) || !finite(kappa)) {
        fail(MG_ERR_ARG, "%s: kappa = %g must be finite and >= 0", who, kappa);
        return false;
    }
    return true;
}
}  // namespace

void mg_newton_opts_default(mg_newton_opts *o)
{
    if (!o) return;
    o->rtol = 1e-8;
    o->atol = 0.0;
    o->max_iters = 20;
    o->max_backtracks = 12;
}

int mg_solver_newton(mg_solver *s, int kind, double kappa, const double *w_dev, const double *F_dev, double *U_dev,
                     const mg_newton_opts *opts, mg_newton_result *out)
{
    const char *who = "mg_solver_newton";
    mg_newton_result r;
    std::memset(&r, 0, sizeof r);
    auto finish = [&](int status) {
        r.status = status;
        r.n_history = s ? (int)s->nw_hist.size() : 0;
        if (out) *out = r;
        return status;
    };
    if (!require_ready(who)) return finish(MG_ERR_NOT_INIT);
    if (!s || !F_dev || !U_dev) {
        fail(MG_ERR_ARG, "%s: NULL solver or array", who);
        return finish(MG_ERR_ARG);
    }
    if (s->op.react) {
        fail(MG_ERR_UNSUPPORTED, "%s: a reaction term is set; the driver installs the Newton matrix's own (take yours away with "
                                 "mg_solver_set_reaction(NULL), or put it into w)", who);
        return finish(MG_ERR_UNSUPPORTED);
    }
    if (s->op.kind) {
        fail(MG_ERR_UNSUPPORTED, "%s: a boundary with a Neumann side is set; the semilinear solve is built for Dirichlet sides", who);
        return finish(MG_ERR_UNSUPPORTED);
    }
    if (s->o.fmg != 0) {
        fail(MG_ERR_UNSUPPORTED, "%s: the solver was created with fmg = %d; the full-multigrid start is not built for a reaction term",
             who, s->o.fmg);
        return finish(MG_ERR_UNSUPPORTED);
    }
    if (!newton_kind_ok(who, kind, kappa)) return finish(MG_ERR_ARG);
    if (((uintptr_t)F_dev | (uintptr_t)U_dev | (uintptr_t)w_dev) % 16 != 0) {
        fail(MG_ERR_ARG, "%s: F, U and w must be 16-byte aligned", who);
        return finish(MG_ERR_ARG);
    }
    mg_newton_opts o;
    mg_newton_opts_default(&o);
    if (opts) o = *opts;
    if (!(o.rtol >= 0.0) || !(o.atol >= 0.0) || !std::isfinite(o.rtol) || !std::isfinite(o.atol) || o.max_iters < 0 || o.max_backtracks < 0) {
        fail(MG_ERR_ARG, "%s: rtol = %g, atol = %g (non-negative, finite), max_iters = %d, max_backtracks = %d (>= 0 each)", who, o.rtol,
             o.atol, o.max_iters, o.max_backtracks);
        return finish(MG_ERR_ARG);
    }
    const hipStream_t st = ctx().stream;
    const int N = s->N, nl = (int)s->sizes.size();
    const size_t n0 = (size_t)N * N;
    if (!react_storage(s)) return finish(MG_ERR_HIP);
    for (double *&p : s->nw_buf)
        if (!p && !dev_alloc(&p, n0)) return finish(MG_ERR_HIP);
    if (w_dev) {   // one launch, a flag, one read-back, as mg_solver_set_reaction checks s
        if (!MG_HIP(hipMemsetAsync(s->react_flag, 0, sizeof(int), st))) return finish(MG_ERR_HIP);
        k::reaction_check(st, w_dev, n0, s->react_flag);
        if (!MG_HIP(hipMemcpyAsync(s->host_react_flag, s->react_flag, sizeof(int), hipMemcpyDeviceToHost, st)) ||
            !MG_HIP(hipStreamSynchronize(st)))
            return finish(MG_ERR_HIP);
        if (*s->host_react_flag) {
            fail(MG_ERR_ARG, "%s: every value of w must be finite and >= 0 (a negative or not finite value found)", who);
            return finish(MG_ERR_ARG);
        }
    }
    s->nw_hist.clear();
    const LevelConsts &c0 = s->lc[0];
    const double *A = s->op.a(0);
    // cur holds the last accepted iterate, D its right-hand side and react[0] its S; oth, D2 and S2 take the next trial.
    // U_dev is one of (cur, oth): when the call ends on the other one, the iterate is copied home.
    double *cur = U_dev, *oth = s->nw_buf[0], *D = s->nw_buf[1], *D2 = s->nw_buf[2], *dlt = s->nw_buf[4];
    double *&S2 = s->nw_buf[3];
    auto home = [&]() {
        s->op.react = nullptr;
        if (cur == U_dev) return true;
        return MG_HIP(hipMemcpyAsync(U_dev, cur, n0 * sizeof(double), hipMemcpyDeviceToDevice, st)) && MG_HIP(hipStreamSynchronize(st));
    };
    k::newton_residual(st, N, c0.inv, c0.sd, kind, kappa, A, w_dev, cur, nullptr, 0.0, F_dev, nullptr, D, s->react[0], s->part, s->dev_scal);
    if (!read_back(s, st)) return finish(MG_ERR_HIP);
    double rn = s->host_scal[0];
    if (!std::isfinite(rn)) {
        fail(MG_ERR_ARG, "%s: the residual of the start is not finite (%g)", who, rn);
        return finish(MG_ERR_ARG);
    }
    r.res0 = r.res = rn;
    const double tol = std::fmax(o.atol, o.rtol * rn);
    bool stalled = false;
    while (!(rn <= tol) && r.iterations < o.max_iters) {
        for (int l = 0; l + 1 < nl; ++l)
            k::coef_coarsen(st, s->sizes[l], s->react[l], s->sizes[l + 1], s->react[l + 1], restrict_table(s->sizes[l], s->sizes[l + 1]));
        if (!MG_HIP(hipMemsetAsync(dlt, 0, n0 * sizeof(double), st))) {
            (void)home();
            return finish(MG_ERR_HIP);
        }
        s->op.react = &s->react;
        mg_solve_result in;
        const int in_status = mg_solver_solve(s, D, dlt, &in);
        s->op.react = nullptr;
        if (in_status > 0) {
            (void)home();
            return finish(in_status);
        }
        mg_newton_iter it{rn, 0.0, 0, in.cycles, in.converged, in.coarse_capped};
        r.inner_cycles += in.cycles;
        double t = 1.0;
        bool accepted = false;
        for (;;) {
            k::newton_residual(st, N, c0.inv, c0.sd, kind, kappa, A, w_dev, cur, dlt, t, F_dev, oth, D2, S2, s->part, s->dev_scal);
            r.trials += 1;
            if (!read_back(s, st)) {
                (void)home();
                return finish(MG_ERR_HIP);
            }
            const double rt = s->host_scal[0];
            if (std::isfinite(rt) && rt < (1.0 - 1e-4 * t) * rn) {
                std::swap(cur, oth);
                std::swap(D, D2);
                std::swap(s->react[0], S2);
                rn = rt;
                it.res = rt;
                it.t = t;
                accepted = true;
                break;
            }
            it.backtracks += 1;
            if (it.backtracks > o.max_backtracks) break;
            t *= 0.5;
        }
        s->nw_hist.push_back(it);
        if (!accepted) {
            stalled = true;
            break;
        }
        r.iterations += 1;
    }
    if (!home()) return finish(MG_ERR_HIP);
    r.res = rn;
    r.converged = rn <= tol ? 1 : 0;
    return finish(r.converged ? MG_NEWTON_CONVERGED : stalled ? MG_NEWTON_STALLED : MG_NEWTON_NOT_CONVERGED);
}

int mg_solver_newton_history(const mg_solver *s, mg_newton_iter *out, int cap)
{
    if (!s) return 0;
    const int n = (int)s->nw_hist.size();
    for (int i = 0; out && i < n && i < cap; ++i) out[i] = s->nw_hist[i];
    return n;
}

int mg_solver_newton_inner_history(const mg_solver *s, double *out, int cap)
{
    if (!s) return 0;
    const int n = (int)s->history.size();
    for (int i = 0; out && i < n && i < cap; ++i) out[i] = s->history[i];
    return n;
}

int mg_nonlinearResidual(int N, double L, double shift, const double *a_dev, int kind, double kappa, const double *w_dev,
                         const double *U, const double *dlt, double t, const double *F, double *V, double *D, double *S, double *norm_out)
{
    const char *who = "mg_nonlinearResidual";
    if (!require_ready(who)) return MG_ERR_NOT_INIT;
    if (!vc_args_ok(who, N, L, shift, {U, F, D, S}) || !rx_coef_ok(who, a_dev) || !newton_kind_ok(who, kind, kappa)) return MG_ERR_ARG;
    if (((uintptr_t)w_dev | (uintptr_t)dlt | (uintptr_t)V) % 16 != 0 || (dlt && (!V || !std::isfinite(t)))) {
        fail(MG_ERR_ARG, "%s: w, dlt and V must be 16-byte aligned; with dlt, V must be there and t = %g finite", who, t);
        return MG_ERR_ARG;
    }
    const hipStream_t st = ctx().stream;
    const size_t np = k::resnorm_partials(N);
    const double dx2 = spacing_sq(N, L), pts = (double)N * N;
    double *buf = nullptr;   // the partials and, behind them, the norm
    if (!dev_alloc(&buf, np + 1)) return MG_ERR_HIP;
    {
        // (timed for scripts/bench_newton.py: U, F in, D, S out, + a, + w, + dlt in and V out)
        ProfScope ps(dlt ? "newton_step" : "newton_residual", N, pts * (32.0 + (a_dev ? 8.0 : 0.0) + (w_dev ? 8.0 : 0.0) + (dlt ? 16.0 : 0.0)));
        k::newton_residual(st, N, 1.0 / dx2, shift * dx2, kind, kappa, a_dev, w_dev, U, dlt, t, F, dlt ? V : nullptr, D, S, buf, buf + np);
    }
    double host = 0.0;
    const bool ok = MG_HIP(hipMemcpyAsync(&host, buf + np, sizeof(double), hipMemcpyDeviceToHost, st)) && MG_HIP(hipStreamSynchronize(st));
    (void)hipFree(buf);
    if (!ok) return MG_ERR_HIP;
    if (norm_out) *norm_out = host;
    return MG_OK;
}

// ------------------------------------------------------------------ the linearisation at U for mg_adjoint_rx.cpp
// mg_solver_newton's refusals, check of w and first pass, then its coarsening of S; the pass's D goes to nw_buf[1] and is dropped
}  // extern "C"

int mg::solver_newton_linearise(mg_solver *s, const char *who, int kind, double kappa, const double *w_dev, const double *F_dev,
                                const double *U_dev, double *res)
{
    if (s->op.react) {
        fail(MG_ERR_UNSUPPORTED, "%s: a reaction term is set; the driver installs the Newton matrix's own (take yours away with "
                                 "mg_solver_set_reaction(NULL), or put it into w)", who);
        return MG_ERR_UNSUPPORTED;
    }
    if (s->op.kind) {
        fail(MG_ERR_UNSUPPORTED, "%s: a boundary with a Neumann side is set; the semilinear solve is built for Dirichlet sides", who);
        return MG_ERR_UNSUPPORTED;
    }
    if (s->o.fmg != 0) {
        fail(MG_ERR_UNSUPPORTED, "%s: the solver was created with fmg = %d; the full-multigrid start is not built for a reaction term",
             who, s->o.fmg);
        return MG_ERR_UNSUPPORTED;
    }
    if (!newton_kind_ok(who, kind, kappa)) return MG_ERR_ARG;
    const hipStream_t st = ctx().stream;
    const int N = s->N, nl = (int)s->sizes.size();
    const size_t n0 = (size_t)N * N;
    if (!react_storage(s)) return MG_ERR_HIP;
    if (!s->nw_buf[1] && !dev_alloc(&s->nw_buf[1], n0)) return MG_ERR_HIP;
    if (w_dev) {
        if (!MG_HIP(hipMemsetAsync(s->react_flag, 0, sizeof(int), st))) return MG_ERR_HIP;
        k::reaction_check(st, w_dev, n0, s->react_flag);
        if (!MG_HIP(hipMemcpyAsync(s->host_react_flag, s->react_flag, sizeof(int), hipMemcpyDeviceToHost, st)) ||
            !MG_HIP(hipStreamSynchronize(st)))
            return MG_ERR_HIP;
        if (*s->host_react_flag) {
            fail(MG_ERR_ARG, "%s: every value of w must be finite and >= 0 (a negative or not finite value found)", who);
            return MG_ERR_ARG;
        }
    }
    const LevelConsts &c0 = s->lc[0];
    k::newton_residual(st, N, c0.inv, c0.sd, kind, kappa, s->op.a(0), w_dev, U_dev, nullptr, 0.0, F_dev, nullptr, s->nw_buf[1], s->react[0],
                       s->part, s->dev_scal);
    if (!read_back(s, st)) return MG_ERR_HIP;
    const double rn = s->host_scal[0];
    if (res) *res = rn;
    if (!std::isfinite(rn)) {
        fail(MG_ERR_ARG, "%s: the residual of U is not finite (%g)", who, rn);
        return MG_ERR_ARG;
    }
    for (int l = 0; l + 1 < nl; ++l)
        k::coef_coarsen(st, s->sizes[l], s->react[l], s->sizes[l + 1], s->react[l + 1], restrict_table(s->sizes[l], s->sizes[l + 1]));
    s->op.react = &s->react;
    return MG_OK;
}

void mg::solver_drop_reaction(mg_solver *s)
{
    if (s) s->op.react = nullptr;
}

extern "C" {

// ------------------------------------------------------------------ boundary kinds per side (include/mg_bc.h)
namespace {
bool kinds_ok(const char *who, const int *kind)
{
    if (!kind) {
        fail(MG_ERR_ARG, "%s: NULL kind (a host int[4]: S, N, W, E)", who);
        return false;
    }
    for (int i = 0; i < 4; ++i)
        if (kind[i] != MG_BC_DIRICHLET && kind[i] != MG_BC_NEUMANN) {
            fail(MG_ERR_ARG, "%s: kind[%d] = %d is neither MG_BC_DIRICHLET (0) nor MG_BC_NEUMANN (1); Robin and periodic sides "
                             "are not built", who, i, kind[i]);
            return false;
        }
    return true;
}

// mg_boundary_prolongation_table(M, N) in device memory
bool make_bc_table(int M, int N, int **lo_dev, double **w_dev)
{
    std::vector<int> lo((size_t)N);
    std::vector<double> w((size_t)N);
    mg_boundary_prolongation_table(M, N, lo.data(), w.data());
    return dev_alloc(lo_dev, lo.size()) && dev_alloc(w_dev, w.size()) &&
           MG_HIP(hipMemcpy(*lo_dev, lo.data(), lo.size() * sizeof(int), hipMemcpyHostToDevice)) &&
           MG_HIP(hipMemcpy(*w_dev, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
}
}  // namespace

void mg_boundary_prolongation_table(int M, int N, int *lo, double *w)
{
    if (M < 2 || N < 2 || !lo || !w) {
        fail(MG_ERR_ARG, "mg_boundary_prolongation_table: M = %d, N = %d (at least 2 each) or a NULL array", M, N);
        return;
    }
    const double h_f = 1.0 / (double)(N - 1), h_c = 1.0 / (double)(M - 1);
    for (int k = 0; k < N; ++k) {
        int l = (int)std::floor((double)k * h_f / h_c);
        if (l > M - 2) l = M - 2;
        double wt = ((double)k * h_f - (double)l * h_c) / h_c;
        wt = wt < 0.0 ? 0.0 : (wt > 1.0 ? 1.0 : wt);
        lo[k] = l;
        w[k] = wt;
    }
    lo[0] = 0;
    w[0] = 0.0;
    lo[N - 1] = M - 2;
    w[N - 1] = 1.0;
}

int mg_solver_set_boundary(mg_solver *s, const int *kind)
{
    if (!require_ready("mg_solver_set_boundary")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_solver_set_boundary: NULL solver");
        return MG_ERR_ARG;
    }
    if (!kinds_ok("mg_solver_set_boundary", kind)) return MG_ERR_ARG;
    const int neumann = kind[0] + kind[1] + kind[2] + kind[3];
    if (neumann == 0) {   // back to the Dirichlet solver (the tables stay for the next boundary)
        s->op.kind = nullptr;
        s->op.project_coarse = false;
        for (int i = 0; i < 4; ++i) s->bc[i] = 0;
        return MG_OK;
    }
    if (s->o.fmg != 0) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_boundary: the solver was created with fmg = %d; the full-multigrid start is not "
                                 "built for boundary kinds", s->o.fmg);
        return MG_ERR_UNSUPPORTED;
    }
    if (s->kr_m > 0) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_boundary: the Krylov acceleration is on (m = %d); it is not built for boundary "
                                 "kinds", s->kr_m);
        return MG_ERR_UNSUPPORTED;
    }
    if (s->op.react) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_boundary: a reaction term is set; a Neumann side together with a reaction is not "
                                 "built (include/mg_reaction.h)");
        return MG_ERR_UNSUPPORTED;
    }
    const bool singular = neumann == 4 && s->o.shift == 0.0;
    if (singular && !s->mean_on) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_boundary: four Neumann sides with shift == 0 is the singular problem; switch the "
                                 "mean fixing on first (mg_solver_set_mean, include/mg_singular.h)");
        return MG_ERR_UNSUPPORTED;
    }
    if (singular && !s->sing_F) {   // the first singular boundary: the projected right-hand side and the scalars
        const size_t n0 = (size_t)s->N * s->N;
        double *f = nullptr, *sc = nullptr, *h = nullptr;
        if (!dev_alloc(&f, n0) || !dev_alloc(&sc, 4) || !MG_HIP(hipHostMalloc((void **)&h, 4 * sizeof(double), hipHostMallocDefault))) {
            if (f) (void)hipFree(f);    // the solver keeps what it had
            if (sc) (void)hipFree(sc);
            return MG_ERR_HIP;
        }
        if (pool_poison_wanted()) {
            poison_block(f, n0 * sizeof(double));
            (void)MG_HIP(hipStreamSynchronize(ctx().stream));
        }
        s->sing_F = f;
        s->sing_scal = sc;
        s->sing_host = h;
    }
    const int nl = (int)s->sizes.size();
    if (s->bc_lo.empty()) {   // the first boundary: the prolongation tables of the hierarchy
        std::vector<int *> lo(nl - 1, nullptr);
        std::vector<double *> w(nl - 1, nullptr);
        bool ok = true;
        for (int l = 0; l + 1 < nl && ok; ++l) ok = make_bc_table(s->sizes[l + 1], s->sizes[l], &lo[l], &w[l]);
        if (!ok) {   // the solver keeps what it had
            for (int *p : lo) if (p) (void)hipFree(p);
            for (double *p : w) if (p) (void)hipFree(p);
            return MG_ERR_HIP;
        }
        s->bc_lo = lo;
        s->bc_w = w;
    }
    for (int i = 0; i < 4; ++i) s->bc[i] = kind[i];
    s->op.kind = s->bc;
    s->op.project_coarse = singular;
    return MG_OK;
}

int mg_solver_boundary(const mg_solver *s, int *kind_out)
{
    if (kind_out)
        for (int i = 0; i < 4; ++i) kind_out[i] = s ? s->bc[i] : 0;
    return s && s->op.kind ? 1 : 0;
}

// ------------------------------------------------------------------ the pure Neumann problem (include/mg_singular.h)
int mg_solver_set_mean(mg_solver *s, int on, double mean)
{
    if (!require_ready("mg_solver_set_mean")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_solver_set_mean: NULL solver");
        return MG_ERR_ARG;
    }
    if (on && !std::isfinite(mean)) {
        fail(MG_ERR_ARG, "mg_solver_set_mean: mean = %g must be finite", mean);
        return MG_ERR_ARG;
    }
    if (!on && s->op.kind && s->op.project_coarse) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_mean: four Neumann sides with shift == 0 are set, the singular problem, which "
                                 "needs the mean fixed; set another boundary first");
        return MG_ERR_UNSUPPORTED;
    }
    s->mean_on = on != 0;
    s->mean = on ? mean : 0.0;
    return MG_OK;
}

int mg_solver_mean(const mg_solver *s, double *mean_out)
{
    if (mean_out) *mean_out = s ? s->mean : 0.0;
    return s && s->mean_on ? 1 : 0;
}

void mg_solver_singular_info(const mg_solver *s, double *out)
{
    if (!out) return;
    for (int i = 0; i < 3; ++i) out[i] = s ? s->sing_info[i] : 0.0;
}

namespace {
// X (N x N) and the other device arrays of a building block: N >= 3, non-NULL, 16-byte aligned
bool mean_args_ok(const char *who, int N, std::initializer_list<const void *> arrays)
{
    if (N < 3 || N > 46340) {
        fail(MG_ERR_ARG, "%s: N = %d outside [3, 46340]", who, N);
        return false;
    }
    for (const void *a : arrays)
        if (!a || (uintptr_t)a % 16 != 0) {
            fail(MG_ERR_ARG, "%s: a NULL array, or one that is not 16-byte aligned", who);
            return false;
        }
    return true;
}

// mean_w(X) -> scalars[32], mean_w(X) - target -> scalars[33] of the engine, enqueued; false without scratch for the partials
bool enqueue_mean(int N, const double *X, double target, double **part_out)
{
    Context &c = ctx();
    double *part = (double *)scratch_pool().get(k::resnorm_partials(N) * sizeof(double));
    if (!part) return false;
    k::weighted_mean(c.stream, N, X, target, part, c.scalars + 32);
    *part_out = part;
    return true;
}
}  // namespace

void mg_weightedMean(int N, const double *X_dev, double *out_host)
{
    if (!require_ready("mg_weightedMean") || !mean_args_ok("mg_weightedMean", N, {X_dev})) return;
    if (!out_host) {
        fail(MG_ERR_ARG, "mg_weightedMean: NULL out_host");
        return;
    }
    Context &c = ctx();
    double *part = nullptr;
    {
        ProfScope ps("wsum", N, (double)N * N * 8.0);
        if (!enqueue_mean(N, X_dev, 0.0, &part)) return;
    }
    if (MG_HIP(hipMemcpyAsync(c.host_scalars + 32, c.scalars + 32, sizeof(double), hipMemcpyDeviceToHost, c.stream)) &&
        MG_HIP(hipStreamSynchronize(c.stream)))
        *out_host = c.host_scalars[32];
    scratch_pool().put(part);
}

void mg_projectMean(int N, const double *X_in, double mean, double *X_out, double *removed_host)
{
    if (!require_ready("mg_projectMean") || !mean_args_ok("mg_projectMean", N, {X_in, X_out})) return;
    if (!std::isfinite(mean)) {
        fail(MG_ERR_ARG, "mg_projectMean: mean = %g must be finite", mean);
        return;
    }
    Context &c = ctx();
    double *part = nullptr;
    {
        ProfScope ps("wsum", N, (double)N * N * 8.0);
        if (!enqueue_mean(N, X_in, mean, &part)) return;
    }
    {
        ProfScope ps("shift", N, (double)N * N * 16.0);
        k::shift_by(c.stream, N, X_in, c.scalars + 33, X_out);
    }
    if (MG_HIP(hipMemcpyAsync(c.host_scalars + 32, c.scalars + 32, sizeof(double), hipMemcpyDeviceToHost, c.stream)) &&
        MG_HIP(hipStreamSynchronize(c.stream)) && removed_host)
        *removed_host = c.host_scalars[32];
    scratch_pool().put(part);
}

void mg_coarseSolveMean(int N, double L, const int *kind, const double *a_dev, const double *F, double atol, double rtol,
                        int max_iters, double *U_out, double *removed_host)
{
    if (!require_ready("mg_coarseSolveMean") || !mean_args_ok("mg_coarseSolveMean", N, {F, U_out}) ||
        !kinds_ok("mg_coarseSolveMean", kind))
        return;
    if (kind[0] + kind[1] + kind[2] + kind[3] != 4 || !k::gs_relative_fits(N) || (uintptr_t)a_dev % 16 != 0 || !(L > 0.0) ||
        !std::isfinite(L) || !(atol >= 0.0) || !(rtol >= 0.0) || !std::isfinite(atol) || !std::isfinite(rtol) || max_iters < 1) {
        fail(MG_ERR_ARG, "mg_coarseSolveMean: four Neumann sides, 3 <= N = %d < %d, a 16-byte aligned, L > 0, atol, rtol >= 0 and "
                         "finite, max_iters >= 1", N, k::GS_RELATIVE_MAX_N);
        return;
    }
    Context &c = ctx();
    const double dx2 = spacing_sq(N, L);
    if (!MG_HIP(hipMemsetAsync(c.gs_state, 0, 4 * sizeof(int), c.stream))) return;
    k::gauss_seidel_relative_bc_mean(c.stream, N, dx2, 1.0 / dx2, kind, a_dev, U_out, F, atol, rtol, max_iters, c.gs_state, nullptr,
                                     c.scalars + 32);
    if (MG_HIP(hipMemcpyAsync(c.host_scalars + 32, c.scalars + 32, sizeof(double), hipMemcpyDeviceToHost, c.stream)) &&
        MG_HIP(hipStreamSynchronize(c.stream)) && removed_host)
        *removed_host = c.host_scalars[32];
}

void mg_neumannSource(int N, double L, const int *kind, const double *a_dev, const double *F, const double *g, double *F_out)
{
    if (!require_ready("mg_neumannSource") || !vc_args_ok("mg_neumannSource", N, L, 0.0, {F, g, F_out}) ||
        !kinds_ok("mg_neumannSource", kind))
        return;
    if ((uintptr_t)a_dev % 16 != 0) {
        fail(MG_ERR_ARG, "mg_neumannSource: a must be 16-byte aligned");
        return;
    }
    const double h = L / (double)(N - 1);
    k::neumann_source(ctx().stream, N, 2.0 / h, kind, a_dev, F, g, F_out);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_applyOperatorBoundary(int N, double L, double shift, const int *kind, const double *a_dev, const double *U, double *out)
{
    if (!require_ready("mg_applyOperatorBoundary") || !vc_args_ok("mg_applyOperatorBoundary", N, L, shift, {U, out}) ||
        !kinds_ok("mg_applyOperatorBoundary", kind))
        return;
    if ((uintptr_t)a_dev % 16 != 0) {
        fail(MG_ERR_ARG, "mg_applyOperatorBoundary: a must be 16-byte aligned");
        return;
    }
    const double dx2 = spacing_sq(N, L);
    k::apply_bc(ctx().stream, N, 1.0 / dx2, shift * dx2, kind, a_dev, U, out);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_sweepBoundary(int N, double L, double shift, double omega, const int *kind, const double *a_dev, const double *U_in,
                      const double *F, double *U_out)
{
    if (!require_ready("mg_sweepBoundary") || !vc_args_ok("mg_sweepBoundary", N, L, shift, {F, U_out}) ||
        !kinds_ok("mg_sweepBoundary", kind))
        return;
    if (((uintptr_t)U_in | (uintptr_t)a_dev) % 16 != 0 || !(omega > 0.0 && omega <= 1.0)) {
        fail(MG_ERR_ARG, "mg_sweepBoundary: a and U_in must be 16-byte aligned, omega = %g inside (0, 1]", omega);
        return;
    }
    const double dx2 = spacing_sq(N, L);
    k::wjacobi_bc(ctx().stream, N, dx2, shift * dx2, omega, kind, a_dev, U_in, F, U_out);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_residualBoundary(int N, double L, double shift, const int *kind, const double *a_dev, const double *U, const double *F,
                         double *D, int sign)
{
    if (!require_ready("mg_residualBoundary") || !vc_args_ok("mg_residualBoundary", N, L, shift, {U, F, D}) ||
        !kinds_ok("mg_residualBoundary", kind))
        return;
    if ((uintptr_t)a_dev % 16 != 0) {
        fail(MG_ERR_ARG, "mg_residualBoundary: a must be 16-byte aligned");
        return;
    }
    const double dx2 = spacing_sq(N, L);
    k::residual_bc(ctx().stream, N, 1.0 / dx2, shift * dx2, kind, a_dev, U, F, D, sign < 0 ? -1 : +1);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_restrictBoundary(int N, const int *kind, const double *D, int M, double *F_c)
{
    if (!require_ready("mg_restrictBoundary") || !kinds_ok("mg_restrictBoundary", kind)) return;
    if (N < 3 || M < 2 || !D || !F_c) {
        fail(MG_ERR_ARG, "mg_restrictBoundary: N = %d (at least 3), M = %d (at least 2) or a NULL array", N, M);
        return;
    }
    const RestrictTable &t = restrict_table(N, M);   // (refuses a table that leaves the fine grid)
    if (!t.lo) return;
    k::restrict_bc(ctx().stream, N, kind, D, M, F_c, t);
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_prolongAddBoundary(int M, const int *kind, const double *U_c, int N, const double *U_in, double *U_out)
{
    if (!require_ready("mg_prolongAddBoundary") || !kinds_ok("mg_prolongAddBoundary", kind)) return;
    if (N < 3 || M < 2 || !U_c || !U_in || !U_out) {
        fail(MG_ERR_ARG, "mg_prolongAddBoundary: M = %d (at least 2), N = %d (at least 3) or a NULL array", M, N);
        return;
    }
    // (the solver keeps its tables from its first boundary on; this entry point builds the one it needs and lets go of it)
    int *lo = nullptr;
    double *w = nullptr;
    if (make_bc_table(M, N, &lo, &w)) {
        k::prolong_add_bc(ctx().stream, M, kind, U_c, N, U_in, U_out, lo, w);
        (void)MG_HIP(hipStreamSynchronize(ctx().stream));
    }
    if (lo) (void)hipFree(lo);
    if (w) (void)hipFree(w);
}

// ------------------------------------------------------------------ Krylov acceleration (include/mg_krylov.h)
int mg_solver_set_krylov(mg_solver *s, int m)
{
    if (!require_ready("mg_solver_set_krylov")) return MG_ERR_NOT_INIT;
    if (!s || m < 0 || m > MG_KRYLOV_MAX_M) {
        fail(MG_ERR_ARG, "mg_solver_set_krylov: NULL solver, or m = %d outside [0, %d]", m, MG_KRYLOV_MAX_M);
        return MG_ERR_ARG;
    }
    if (s->o.fmg != 0) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_krylov: the solver was created with fmg = %d; the full-multigrid start is not "
                                 "combined with the Krylov acceleration", s->o.fmg);
        return MG_ERR_UNSUPPORTED;
    }
    if (m > 0 && s->op.kind) {
        fail(MG_ERR_UNSUPPORTED, "mg_solver_set_krylov: a boundary with a Neumann side is set; the Krylov acceleration is not built "
                                 "for boundary kinds (its sums and its operator run over the interior)");
        return MG_ERR_UNSUPPORTED;
    }
    const int have = (int)s->kr_Z.size();
    if (m > have) {   // the additional slots, and with the first of them r, the partials, the scalars and the log
        const size_t n = (size_t)s->N * s->N;
        const size_t n_part = (size_t)k::KRYLOV_MAX_K * k::krylov_blocks(s->N);
        const size_t n_log = (size_t)(s->o.max_cycles > 0 ? s->o.max_cycles : 1) * KR_REC_MAX;
        const bool first = s->kr_r == nullptr;
        std::vector<double *> Z, Q;
        double *r = nullptr, *part = nullptr, *scal = nullptr, *log = nullptr, *host = nullptr;
        bool ok = true;
        if (first)
            ok = dev_alloc(&r, n) && dev_alloc(&part, n_part) && dev_alloc(&scal, (size_t)KR_SCALARS) && dev_alloc(&log, n_log) &&
                 MG_HIP(hipHostMalloc((void **)&host, 2 * sizeof(double), hipHostMallocDefault)) &&
                 MG_HIP(hipMemset(scal, 0, KR_SCALARS * sizeof(double)));
        for (int j = have; j < m && ok; ++j) {
            double *z = nullptr, *q = nullptr;
            ok = dev_alloc(&z, n);
            if (ok) Z.push_back(z);
            ok = ok && dev_alloc(&q, n);
            if (ok) Q.push_back(q);
        }
        if (!ok) {   // the solver keeps what it had
            for (double *p : Z) (void)hipFree(p);
            for (double *p : Q) (void)hipFree(p);
            for (double *p : {r, part, scal, log}) if (p) (void)hipFree(p);
            if (host) (void)hipHostFree(host);
            return MG_ERR_HIP;
        }
        if (pool_poison_wanted()) {   // MG_POOL_POISON: no array starts from what hipMalloc happened to return
            for (double *p : Z) poison_block(p, n * sizeof(double));
            for (double *p : Q) poison_block(p, n * sizeof(double));
            if (first) {
                poison_block(r, n * sizeof(double));
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
            s->kr_host = host;
            s->kr_host[0] = s->kr_host[1] = 0.0;
            s->kr_log_host.assign(n_log, 0.0);
        }
        s->kr_Z.insert(s->kr_Z.end(), Z.begin(), Z.end());
        s->kr_Q.insert(s->kr_Q.end(), Q.begin(), Q.end());
    }
    s->kr_m = m;
    return MG_OK;
}

int mg_solver_krylov(const mg_solver *s) { return s ? s->kr_m : 0; }

int mg_solver_krylov_breakdown(const mg_solver *s) { return s && s->kr_m > 0 && s->kr_breakdown ? 1 : 0; }

int mg_solver_krylov_log(const mg_solver *s, double *out, int cap)
{
    if (!s) return 0;
    if (!out) return s->kr_records;
    const int n = cap < s->kr_records ? (cap > 0 ? cap : 0) : s->kr_records;
    if (n > 0) std::memcpy(out, s->kr_log_host.data(), (size_t)n * (s->kr_log_m + 7) * sizeof(double));
    return n;
}

namespace {
bool krylov_hook_ok(const char *who, int N, int k, std::initializer_list<const void *> arrays)
{
    if (N < 3 || k < 0 || k > k::KRYLOV_MAX_K) {
        fail(MG_ERR_ARG, "%s: N = %d (at least 3), k = %d (0 .. %d)", who, N, k, k::KRYLOV_MAX_K);
        return false;
    }
    for (const void *p : arrays)
        if (!p || (uintptr_t)p % 16 != 0) {
            fail(MG_ERR_ARG, "%s: a NULL or not 16-byte aligned array", who);
            return false;
        }
    return true;
}
}  // namespace

void mg_krylovDots(int N, int k, const double *q, const double *const *Q, double *out)
{
    if (!require_ready("mg_krylovDots") || !krylov_hook_ok("mg_krylovDots", N, k, {q})) return;
    if (k == 0) return;
    if (!Q || !out) {
        fail(MG_ERR_ARG, "mg_krylovDots: NULL Q or out");
        return;
    }
    k::KrylovVecs v{};
    for (int j = 0; j < k; ++j) {
        if (!krylov_hook_ok("mg_krylovDots", N, k, {Q[j]})) return;
        v.q[j] = Q[j];
    }
    Context &c = ctx();
    double *part = partials((size_t)k * k::krylov_blocks(N));
    if (!part) return;
    {
        ProfScope ps("krylov_dots", N, (double)N * N * (8.0 + 8.0 * k));
        k::krylov_dots(c.stream, N, k, q, v, part, nullptr, nullptr, c.scalars);
    }
    if (MG_HIP(hipMemcpyAsync(c.host_scalars, c.scalars, k * sizeof(double), hipMemcpyDeviceToHost, c.stream)) &&
        MG_HIP(hipStreamSynchronize(c.stream)))
        std::memcpy(out, c.host_scalars, k * sizeof(double));
}

void mg_krylovOrth(int N, int k, const double *b, double *q, double *z, const double *r, const double *const *Q,
                   const double *const *Z, double *gh)
{
    if (!require_ready("mg_krylovOrth") || !krylov_hook_ok("mg_krylovOrth", N, k, {q, z, r})) return;
    if (!gh || (k > 0 && (!b || !Q || !Z))) {
        fail(MG_ERR_ARG, "mg_krylovOrth: NULL b, Q, Z or gh");
        return;
    }
    k::KrylovVecs v{};
    for (int j = 0; j < k; ++j) {
        if (!krylov_hook_ok("mg_krylovOrth", N, k, {Q[j], Z[j]})) return;
        v.q[j] = Q[j];
        v.z[j] = Z[j];
    }
    Context &c = ctx();
    double *part = partials(2 * k::krylov_blocks(N));
    if (!part) return;
    // b at scalars[0 .. k), g and h at scalars[16 .. 18)
    if (k > 0) {
        std::memcpy(c.host_scalars, b, k * sizeof(double));
        if (!MG_HIP(hipMemcpyAsync(c.scalars, c.host_scalars, k * sizeof(double), hipMemcpyHostToDevice, c.stream))) return;
    }
    {
        ProfScope ps("krylov_orth", N, (double)N * N * (k > 0 ? 40.0 + 16.0 * k : 16.0));
        k::krylov_orth(c.stream, N, k, q, z, r, v, c.scalars, part);
    }
    k::krylov_orth_finish(c.stream, N, part, k, 0, c.scalars + 16, nullptr, nullptr, nullptr, nullptr);
    if (!MG_HIP(hipStreamSynchronize(c.stream))) return;   // (host_scalars is free again)
    if (MG_HIP(hipMemcpyAsync(c.host_scalars, c.scalars + 16, 2 * sizeof(double), hipMemcpyDeviceToHost, c.stream)) &&
        MG_HIP(hipStreamSynchronize(c.stream)))
        std::memcpy(gh, c.host_scalars, 2 * sizeof(double));
}

void mg_krylovUpdate(int N, double alpha, double *U, const double *z, double *r, const double *q, double *rr)
{
    if (!require_ready("mg_krylovUpdate") || !krylov_hook_ok("mg_krylovUpdate", N, 0, {U, z, r, q})) return;
    if (!rr) {
        fail(MG_ERR_ARG, "mg_krylovUpdate: NULL rr");
        return;
    }
    Context &c = ctx();
    double *part = partials(k::krylov_blocks(N));
    if (!part) return;
    c.host_scalars[0] = alpha;
    if (!MG_HIP(hipMemcpyAsync(c.scalars, c.host_scalars, sizeof(double), hipMemcpyHostToDevice, c.stream))) return;
    {
        ProfScope ps("krylov_update", N, (double)N * N * 48.0);
        k::krylov_update(c.stream, N, c.scalars, U, z, r, q, part);
    }
    k::krylov_update_finish(c.stream, N, part, c.scalars + 16, nullptr, nullptr);
    if (!MG_HIP(hipStreamSynchronize(c.stream))) return;
    if (MG_HIP(hipMemcpyAsync(c.host_scalars, c.scalars + 16, sizeof(double), hipMemcpyDeviceToHost, c.stream)) &&
        MG_HIP(hipStreamSynchronize(c.stream)))
        *rr = c.host_scalars[0];
}

void mg_solver_destroy(mg_solver *s)
{
    if (!s) return;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    release(s);
}

}  // extern "C"
