// mg_adjoint_rx.cpp -- the adjoint of reaction and semilinear solves (include/mg_adjoint_rx.h).  The linearisation of either
// problem at its solution is the symmetric reaction operator the solver already has, so the adjoint solve is mg_solver_solve on
// the right-hand side Ubar from the zero field; what this file adds is thin, as mg_adjoint.cpp: the argument checks, the source
// gradient (mg_adjoint_rx_kernels.hip) and the drivers that chain {zero fill, solve, coefficient gradient, rim gradient,
// source gradient} on the engine stream.  A driver enqueues exactly what the caller's own sequence of the public functions
// enqueues, so its bits are that sequence's.  The semilinear driver takes its Newton matrix from mg_solve.cpp
// (solver_newton_linearise: the no-step pass and the coarsening of mg_solver_newton) and leaves the solver without a reaction.
// The partials of a sum and the sum itself come from the scratch pool for the length of a call.
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "mg_internal.h"

using namespace mg;

namespace {

bool overlap(const void *a, const void *b, size_t bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

bool aligned(const void *p) { return (uintptr_t)p % 16 == 0; }

double level0_inv(int N, double L)
{
    mg_solve_opts so;
    mg_solve_opts_default(&so);
    return solve_level_consts(std::vector<int>{N}, L, so)[0].inv;
}

bool kind_ok(const char *who, int N, int kind, double kappa)
{
    if (N < 3) {
        fail(MG_ERR_ARG, "%s: N = %d (at least 3)", who, N);
        return false;
    }
    if (kind != MG_NEWTON_CUBIC && kind != MG_NEWTON_SINH && kind != MG_NEWTON_EXP && kind != MG_GRAD_LINEAR) {
        fail(MG_ERR_ARG, "%s: unknown kind %d (MG_NEWTON_CUBIC = 0, MG_NEWTON_SINH = 1, MG_NEWTON_EXP = 2, MG_GRAD_LINEAR = 3)", who, kind);
        return false;
    }
    if (!std::isfinite(kappa)) {
        fail(MG_ERR_ARG, "%s: kappa = %g must be finite", who, kappa);
        return false;
    }
    return true;
}

// every output against every input and against every other output (nullptr entries: not given); false after fail
bool no_overlap(const char *who, int N, const std::vector<const void *> &ins, const std::vector<const void *> &outs)
{
    const size_t bytes = (size_t)N * N * sizeof(double);
    for (size_t i = 0; i < outs.size(); ++i) {
        if (!outs[i]) continue;
        for (const void *p : ins)
            if (p && overlap(outs[i], p, bytes)) {
                fail(MG_ERR_ARG, "%s: an output array overlaps an input array", who);
                return false;
            }
        for (size_t j = i + 1; j < outs.size(); ++j)
            if (outs[j] && overlap(outs[i], outs[j], bytes)) {
                fail(MG_ERR_ARG, "%s: two output arrays overlap", who);
                return false;
            }
    }
    return true;
}

// `count` doubles from the scratch pool for the length of a call
struct Scratch {
    double *dev = nullptr;
    explicit Scratch(size_t count) { dev = static_cast<double *>(scratch_pool().get(count * sizeof(double))); }
    ~Scratch()
    {
        if (dev) scratch_pool().put(dev);
    }
};

double src_bytes(int N, bool has_w) { return (double)N * N * (has_w ? 32.0 : 24.0); }   // lam, U (, w) read, G written

// the tail of both drivers: the gradients of a finished adjoint solve, then the one synchronisation.  sum: host, may be NULL
int gradients(const char *who, mg_solver *s, int status, int kind, double kappa, const double *w, const double *Ubar, const double *U,
              const double *lam, double *gA, double *gU, double *gG, double *sum, mg_solve_result *out)
{
    if (!gA && !gU && !gG) return status;   // (just the solve, which has synchronised)
    double L = 1.0;
    const int N = solver_size(s, &L);
    const hipStream_t st = ctx().stream;
    const double inv = level0_inv(N, L);
    const size_t np = k::resnorm_partials(N);
    Scratch sc(gG ? np + 1 : 1);
    auto hip_failed = [&]() {
        if (out) out->status = MG_ERR_HIP;
        return MG_ERR_HIP;
    };
    if (gG && !sc.dev) {
        fail(MG_ERR_HIP, "%s: no scratch memory for the partial sums", who);
        return hip_failed();
    }
    if (gA) {
        ProfScope ps("coef_grad", N, (double)N * N * 24.0);
        k::coef_grad(st, N, 0.5 * inv, lam, U, gA);
    }
    if (gU) {
        ProfScope ps("rim_grad", N, (double)N * N * 8.0);
        k::rim_grad(st, N, inv, solver_coefficient(s), lam, Ubar, gU);
    }
    double host = 0.0;
    if (gG) {
        {
            ProfScope ps(w ? "src_grad_w" : "src_grad", N, src_bytes(N, w != nullptr));
            k::src_grad(st, N, kind, kappa, w, lam, U, gG, sc.dev, sc.dev + np);
        }
        if (sum && !MG_HIP(hipMemcpyAsync(&host, sc.dev + np, sizeof(double), hipMemcpyDeviceToHost, st))) return hip_failed();
    }
    if (!MG_HIP(hipStreamSynchronize(st))) return hip_failed();
    if (gG && sum) *sum = host;
    return status;
}

// Both batched drivers.  newton: the semilinear form (kind, kappa, n_w, w, F and res_forward are its own); else the reaction
// form, whose source gradient is MG_GRAD_LINEAR at kappa = 1 without a weight.  Every table -- the coefficient gradient's,
// the rim gradient's, the source gradient's -- and the partials come from ONE scratch block and are uploaded before the solve:
// every address in them is known up front.  The three gradient launches and the finish run once over all n instances.
int batch_adjoint(const char *who, mg_batch_solver *s, int n, bool newton, int kind, const double *kappa, int n_w, const double *const *w,
                  const double *const *F, const double *const *U, const double *const *Ubar, double *const *lam, double *const *gA,
                  double *const *gU, double *const *gG, double *sums, double *res_forward, mg_solve_result *out, mg_batch_solve_stats *stats)
{
    int max_batch = 0, N = 0;
    double L = 1.0;
    auto refuse = [&](int code) {
        if (out && s && n >= 1 && n <= max_batch)
            for (int i = 0; i < n; ++i) {
                std::memset(&out[i], 0, sizeof out[i]);
                out[i].status = code;
            }
        if (stats) std::memset(stats, 0, sizeof *stats);
        return code;
    };
    if (!require_ready(who)) return refuse(MG_ERR_NOT_INIT);
    const bool needs_u = newton || gA || gG;
    if (!s || !Ubar || !lam || !out || (needs_u && !U) || (sums && !gG) || (newton && (!F || !kappa))) {
        fail(MG_ERR_ARG, "%s: NULL solver, Ubar, lam or result array, a gradient wanted without U, or a sum wanted without its gradient", who);
        return refuse(MG_ERR_ARG);
    }
    N = batch_solver_size(s, &L, &max_batch);
    if (n < 1 || n > max_batch) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, max_batch = %d]", who, n, max_batch);
        return refuse(MG_ERR_ARG);
    }
    const int n_coef = mg_batch_solver_has_coefficient(s), n_react = mg_batch_solver_has_reaction(s);
    if ((n_coef > 1 && n > n_coef) || (n_react > 1 && n > n_react)) {
        fail(MG_ERR_ARG, "%s: n = %d instances, but the solver holds %d coefficients and %d reaction terms (one per instance)", who, n, n_coef,
             n_react);
        return refuse(MG_ERR_ARG);
    }
    if (newton && !(n_w == 0 || n_w == 1 || n_w == n)) {   // (the entries: batch_solver_newton_linearise)
        fail(MG_ERR_ARG, "%s: %d w arrays for %d instances (0: none, 1: one shared by all, or one per instance)", who, n_w, n);
        return refuse(MG_ERR_ARG);
    }
    const bool has_w = newton && n_w > 0 && w;
    std::vector<NodeBatchItem> tab((size_t)2 * n);   // [0, n): the coefficient gradient; [n, 2n): the rim gradient
    std::vector<k::SrcGradItem> src(n);
    std::vector<const void *> ins, outs;
    for (int i = 0; i < n; ++i) {
        const double *u = needs_u ? U[i] : nullptr, *coef = batch_solver_coefficient(s, i), *f = newton ? F[i] : nullptr;
        const double *wi = has_w ? w[n_w == 1 ? 0 : i] : nullptr;
        double *ga = gA ? gA[i] : nullptr, *gu = gU ? gU[i] : nullptr, *gg = gG ? gG[i] : nullptr;
        if (!Ubar[i] || !lam[i] || (needs_u && !u) || (gA && !ga) || (gU && !gu) || (gG && !gg) || (newton && !f)) {
            fail(MG_ERR_ARG, "%s: a NULL array of instance %d", who, i);
            return refuse(MG_ERR_ARG);
        }
        if (!aligned(Ubar[i]) || !aligned(lam[i]) || !aligned(u) || !aligned(ga) || !aligned(gu) || !aligned(gg) || !aligned(f) || !aligned(wi)) {
            fail(MG_ERR_ARG, "%s: every array of instance %d must be 16-byte aligned", who, i);
            return refuse(MG_ERR_ARG);
        }
        for (const void *p : {(const void *)(gU ? coef : nullptr), (const void *)Ubar[i], (const void *)u, (const void *)f, (const void *)wi})
            ins.push_back(p);
        for (const void *p : {(const void *)lam[i], (const void *)ga, (const void *)gu, (const void *)gg}) outs.push_back(p);
        tab[i] = NodeBatchItem{lam[i], u, nullptr, ga, nullptr};
        tab[(size_t)n + i] = NodeBatchItem{lam[i], Ubar[i], coef, gu, nullptr};
        src[i] = k::SrcGradItem{wi, lam[i], u, gg, newton ? kappa[i] : 1.0};
    }
    if (!no_overlap(who, N, ins, outs)) return refuse(MG_ERR_ARG);
    mg_batch_solve_stats bs;
    std::memset(&bs, 0, sizeof bs);
    int extra = 0;   // launches outside the solve
    if (newton) {
        const int lin = batch_solver_newton_linearise(s, who, n, kind, kappa, n_w, w, F, U, res_forward, &extra);
        if (lin != MG_OK) return refuse(lin);
    }
    const hipStream_t st = ctx().stream;
    const size_t np = k::resnorm_partials(N), sum_doubles = gG ? (size_t)n * np + n : 0;
    const size_t tab_bytes = tab.size() * sizeof(NodeBatchItem), src_bytes_ = src.size() * sizeof(k::SrcGradItem);
    Scratch sc(sum_doubles + (tab_bytes + src_bytes_) / sizeof(double) + 1);
    auto fail_hip = [&]() {
        if (newton) batch_solver_drop_reaction(s);
        return refuse(MG_ERR_HIP);
    };
    if (!sc.dev) {
        fail(MG_ERR_HIP, "%s: no scratch memory for the tables and the partial sums", who);
        return fail_hip();
    }
    NodeBatchItem *tab_dev = reinterpret_cast<NodeBatchItem *>(sc.dev + sum_doubles);
    k::SrcGradItem *src_dev = reinterpret_cast<k::SrcGradItem *>(tab_dev + tab.size());
    if ((gA || gU) && !MG_HIP(hipMemcpyAsync(tab_dev, tab.data(), tab_bytes, hipMemcpyHostToDevice, st))) return fail_hip();
    if (gG && !MG_HIP(hipMemcpyAsync(src_dev, src.data(), src_bytes_, hipMemcpyHostToDevice, st))) return fail_hip();
    for (int i = 0; i < n; ++i)
        if (!MG_HIP(hipMemsetAsync(lam[i], 0, (size_t)N * N * sizeof(double), st))) return fail_hip();
    const int status = mg_batch_solver_solve(s, n, Ubar, lam, out, &bs);
    if (newton) batch_solver_drop_reaction(s);
    bs.launches += extra;
    std::vector<double> host(n, 0.0);
    if (status <= 0 && (gA || gU || gG)) {
        const double inv = level0_inv(N, L);
        bool ok = true;
        if (gA) {
            ProfScope ps("coef_grad_batch", N, (double)N * N * 24.0 * n);
            k::coef_grad_batch(st, n, N, 0.5 * inv, tab_dev);
            bs.launches += 1;
        }
        if (gU) {
            ProfScope ps("rim_grad_batch", N, (double)N * N * 8.0 * n);
            k::rim_grad_batch(st, n, N, inv, tab_dev + n);
            bs.launches += 1;
        }
        if (gG) {
            {
                ProfScope ps(has_w ? "src_grad_w_batch" : "src_grad_batch", N, src_bytes(N, has_w) * n);
                k::src_grad_batch(st, n, N, newton ? kind : MG_GRAD_LINEAR, has_w, src_dev, sc.dev, sc.dev + (size_t)n * np);
            }
            bs.launches += 2;
            if (sums) ok = MG_HIP(hipMemcpyAsync(host.data(), sc.dev + (size_t)n * np, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        if (!ok || !MG_HIP(hipStreamSynchronize(st))) {
            for (int i = 0; i < n; ++i) out[i].status = MG_ERR_HIP;
            if (stats) *stats = bs;
            return MG_ERR_HIP;
        }
        if (gG && sums) std::memcpy(sums, host.data(), (size_t)n * sizeof(double));
    }
    if (stats) *stats = bs;
    return status;
}

}  // namespace

extern "C" {

int mg_batch_solver_adjoint_reaction(mg_batch_solver *s, int n, const double *const *Ubar, const double *const *U, double *const *lam,
                                     double *const *gA, double *const *gU, double *const *gS, double *gshift, mg_solve_result *out,
                                     mg_batch_solve_stats *stats)
{
    return batch_adjoint("mg_batch_solver_adjoint_reaction", s, n, false, MG_GRAD_LINEAR, nullptr, 0, nullptr, nullptr, U, Ubar, lam, gA, gU, gS,
                         gshift, nullptr, out, stats);
}

int mg_batch_solver_newton_adjoint(mg_batch_solver *s, int n, int kind, const double *kappa, int n_w, const double *const *w,
                                   const double *const *F, const double *const *U, const double *const *Ubar, double *const *lam,
                                   double *const *gA, double *const *gU, double *const *gW, double *gkappa, double *res_forward,
                                   mg_solve_result *out, mg_batch_solve_stats *stats)
{
    return batch_adjoint("mg_batch_solver_newton_adjoint", s, n, true, kind, kappa, n_w, w, F, U, Ubar, lam, gA, gU, gW, gkappa, res_forward,
                         out, stats);
}

int mg_sourceGradient(int N, int kind, double kappa, const double *w, const double *lam, const double *U, double *G, double *sum)
{
    const char *who = "mg_sourceGradient";
    if (!require_ready(who)) return MG_ERR_NOT_INIT;
    if (!kind_ok(who, N, kind, kappa)) return MG_ERR_ARG;
    if (!lam || !U || !G || !aligned(lam) || !aligned(U) || !aligned(G) || !aligned(w)) {
        fail(MG_ERR_ARG, "%s: a NULL lam, U or G, or an array that is not 16-byte aligned", who);
        return MG_ERR_ARG;
    }
    if (!no_overlap(who, N, {w, lam, U}, {G})) return MG_ERR_ARG;
    const hipStream_t st = ctx().stream;
    const size_t np = k::resnorm_partials(N);
    Scratch sc(np + 1);
    if (!sc.dev) {
        fail(MG_ERR_HIP, "%s: no scratch memory for the partial sums", who);
        return MG_ERR_HIP;
    }
    {
        ProfScope ps(w ? "src_grad_w" : "src_grad", N, src_bytes(N, w != nullptr));   // (scripts/bench_adjoint_rx.py)
        k::src_grad(st, N, kind, kappa, w, lam, U, G, sc.dev, sc.dev + np);
    }
    double host = 0.0;
    if (sum && !MG_HIP(hipMemcpyAsync(&host, sc.dev + np, sizeof(double), hipMemcpyDeviceToHost, st))) return MG_ERR_HIP;
    if (!MG_HIP(hipStreamSynchronize(st))) return MG_ERR_HIP;
    if (sum) *sum = host;
    return MG_OK;
}

int mg_sourceGradient_batch(int n, int N, int kind, const double *kappa, int n_w, const double *const *w, const double *const *lam,
                            const double *const *U, double *const *G, double *sums)
{
    const char *who = "mg_sourceGradient_batch";
    if (!require_ready(who)) return MG_ERR_NOT_INIT;
    if (n < 1 || n > 65535 || !kappa || !lam || !U || !G) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, 65535], or a NULL kappa or pointer array", who, n);
        return MG_ERR_ARG;
    }
    if (!(n_w == 0 || n_w == 1 || n_w == n) || (n_w == 0) != (w == nullptr)) {
        fail(MG_ERR_ARG, "%s: n_w = %d must be 0 (w == NULL), 1 (shared) or n = %d", who, n_w, n);
        return MG_ERR_ARG;
    }
    std::vector<k::SrcGradItem> tab(n);
    std::vector<const void *> ins, outs;
    for (int i = 0; i < n; ++i) {
        if (!kind_ok(who, N, kind, kappa[i])) return MG_ERR_ARG;
        const double *wi = n_w == 0 ? nullptr : w[n_w == 1 ? 0 : i];
        if (!lam[i] || !U[i] || !G[i] || (n_w && !wi) || !aligned(lam[i]) || !aligned(U[i]) || !aligned(G[i]) || !aligned(wi)) {
            fail(MG_ERR_ARG, "%s: a NULL or not 16-byte aligned array of instance %d", who, i);
            return MG_ERR_ARG;
        }
        tab[i] = k::SrcGradItem{wi, lam[i], U[i], G[i], kappa[i]};
        for (const void *p : {(const void *)wi, (const void *)lam[i], (const void *)U[i]}) ins.push_back(p);
        outs.push_back(G[i]);
    }
    if (!no_overlap(who, N, ins, outs)) return MG_ERR_ARG;
    const hipStream_t st = ctx().stream;
    const size_t np = k::resnorm_partials(N), tab_doubles = ((size_t)n * sizeof(k::SrcGradItem) + sizeof(double) - 1) / sizeof(double);
    // one block: the partials of every instance, the n sums, the table (8-byte items behind doubles: aligned)
    Scratch sc((size_t)n * np + n + tab_doubles);
    if (!sc.dev) {
        fail(MG_ERR_HIP, "%s: no scratch memory for the partial sums", who);
        return MG_ERR_HIP;
    }
    double *out_dev = sc.dev + (size_t)n * np;
    k::SrcGradItem *tab_dev = reinterpret_cast<k::SrcGradItem *>(out_dev + n);
    if (!MG_HIP(hipMemcpyAsync(tab_dev, tab.data(), (size_t)n * sizeof(k::SrcGradItem), hipMemcpyHostToDevice, st))) return MG_ERR_HIP;
    {
        ProfScope ps(n_w ? "src_grad_w_batch" : "src_grad_batch", N, src_bytes(N, n_w != 0) * n);
        k::src_grad_batch(st, n, N, kind, n_w != 0, tab_dev, sc.dev, out_dev);
    }
    std::vector<double> host(n, 0.0);
    if (sums && !MG_HIP(hipMemcpyAsync(host.data(), out_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st))) return MG_ERR_HIP;
    if (!MG_HIP(hipStreamSynchronize(st))) return MG_ERR_HIP;
    if (sums) std::memcpy(sums, host.data(), (size_t)n * sizeof(double));
    return MG_OK;
}

int mg_solver_adjoint_reaction(mg_solver *s, const double *Ubar, const double *U, double *lam, double *gA, double *gU, double *gS,
                               double *gshift, mg_solve_result *out)
{
    const char *who = "mg_solver_adjoint_reaction";
    auto refuse = [&](int code) {
        if (out) {
            std::memset(out, 0, sizeof *out);
            out->status = code;
        }
        return code;
    };
    if (!require_ready(who)) return refuse(MG_ERR_NOT_INIT);
    if (!s || !Ubar || !lam || ((gA || gS) && !U) || (gshift && !gS)) {
        fail(MG_ERR_ARG, "%s: NULL solver, Ubar or lam, gA or gS wanted without U, or gshift wanted without gS", who);
        return refuse(MG_ERR_ARG);
    }
    if (!aligned(Ubar) || !aligned(U) || !aligned(lam) || !aligned(gA) || !aligned(gU) || !aligned(gS)) {
        fail(MG_ERR_ARG, "%s: every array must be 16-byte aligned", who);
        return refuse(MG_ERR_ARG);
    }
    if (solver_boundary(s)) {   // (include/mg_bc.h: the gradient kernels treat the whole rim as data)
        fail(MG_ERR_UNSUPPORTED, "%s: a boundary with a Neumann side is set; the adjoint is not built for boundary kinds", who);
        return refuse(MG_ERR_UNSUPPORTED);
    }
    const int N = solver_size(s, nullptr);
    if (!no_overlap(who, N, {gU ? solver_coefficient(s) : nullptr, Ubar, gA || gS ? U : nullptr}, {lam, gA, gU, gS})) return refuse(MG_ERR_ARG);
    const hipStream_t st = ctx().stream;
    if (!MG_HIP(hipMemsetAsync(lam, 0, (size_t)N * N * sizeof(double), st))) return refuse(MG_ERR_HIP);   // mg_fill_zero
    const int status = mg_solver_solve(s, Ubar, lam, out);
    if (status > 0) return status;
    return gradients(who, s, status, MG_GRAD_LINEAR, 1.0, nullptr, Ubar, U, lam, gA, gU, gS, gshift, out);
}

int mg_solver_newton_adjoint(mg_solver *s, int kind, double kappa, const double *w, const double *F, const double *U, const double *Ubar,
                             double *lam, double *gA, double *gU, double *gW, double *gkappa, double *res_forward, mg_solve_result *out)
{
    const char *who = "mg_solver_newton_adjoint";
    auto refuse = [&](int code) {
        if (out) {
            std::memset(out, 0, sizeof *out);
            out->status = code;
        }
        return code;
    };
    if (!require_ready(who)) return refuse(MG_ERR_NOT_INIT);
    if (!s || !F || !U || !Ubar || !lam || (gkappa && !gW)) {
        fail(MG_ERR_ARG, "%s: NULL solver, F, U, Ubar or lam, or gkappa wanted without gW", who);
        return refuse(MG_ERR_ARG);
    }
    if (!aligned(w) || !aligned(F) || !aligned(U) || !aligned(Ubar) || !aligned(lam) || !aligned(gA) || !aligned(gU) || !aligned(gW)) {
        fail(MG_ERR_ARG, "%s: every array must be 16-byte aligned", who);
        return refuse(MG_ERR_ARG);
    }
    const int N = solver_size(s, nullptr);
    if (!no_overlap(who, N, {solver_coefficient(s), w, F, U, Ubar}, {lam, gA, gU, gW})) return refuse(MG_ERR_ARG);
    const int lin = solver_newton_linearise(s, who, kind, kappa, w, F, U, res_forward);
    if (lin != MG_OK) return refuse(lin);
    const hipStream_t st = ctx().stream;
    if (!MG_HIP(hipMemsetAsync(lam, 0, (size_t)N * N * sizeof(double), st))) {
        solver_drop_reaction(s);
        return refuse(MG_ERR_HIP);
    }
    const int status = mg_solver_solve(s, Ubar, lam, out);
    solver_drop_reaction(s);
    if (status > 0) return status;
    return gradients(who, s, status, kind, kappa, w, Ubar, U, lam, gA, gU, gW, gkappa, out);
}

}  // extern "C"
