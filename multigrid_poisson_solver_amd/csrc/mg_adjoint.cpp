// mg_adjoint.cpp -- adjoint sensitivities over the residual-tolerance solvers (include/mg_adjoint.h).  The operator is
// symmetric on the interior, so the adjoint solve is mg_solver_solve / mg_batch_solver_solve on the right-hand side Ubar from
// the zero field; what this file adds is thin: the argument checks, the two contractions that turn the adjoint field into
// gradients (mg_adjoint_kernels.hip) and the drivers that chain {zero fill, solve, coefficient gradient, rim gradient} on the
// engine stream.  A driver enqueues exactly what the caller's own sequence of the public functions enqueues, so its bits
// are that sequence's; the host synchronises where the solve does and once at the end.  The tables of the batched
// launches come from the scratch pool and are uploaded BEFORE the solve: every address in them is known up front.
#include <cmath>
#include <cstring>
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

// the level-0 constant of the solvers (include/mg_hip.h): inv = 1/dx2, dx2 = (L/(N-1))^2
double level0_inv(int N, double L)
{
    mg_solve_opts so;
    mg_solve_opts_default(&so);
    return solve_level_consts(std::vector<int>{N}, L, so)[0].inv;
}

bool shape_ok(const char *who, int N, double L)
{
    if (N < 3 || !(L > 0.0) || !std::isfinite(L)) {
        fail(MG_ERR_ARG, "%s: N = %d (at least 3), L = %g (positive, finite)", who, N, L);
        return false;
    }
    return true;
}

double grad_bytes(int N) { return (double)N * N * 24.0; }   // lam, U read, gA written
double rim_bytes(int N) { return (double)N * N * 8.0; }     // gU written; O(N) more

// One instance's arrays of an adjoint call; nullptr where an array is not given / not wanted.
struct Arrays {
    const double *a, *Ubar, *U;
    double *lam, *gA, *gU;
};

// every output against every input of every instance and against every other output; false after fail.
// lam_is_output: the drivers write lam; for the point functions it is an input
bool no_overlap(const char *who, int N, const std::vector<Arrays> &x, bool lam_is_output)
{
    const size_t bytes = (size_t)N * N * sizeof(double);
    std::vector<const void *> ins, outs;
    for (const Arrays &v : x) {
        for (const double *p : {v.a, v.Ubar, v.U})
            if (p) ins.push_back(p);
        if (v.lam) (lam_is_output ? outs : ins).push_back(v.lam);
        for (double *p : {v.gA, v.gU})
            if (p) outs.push_back(p);
    }
    for (size_t i = 0; i < outs.size(); ++i) {
        for (const void *p : ins)
            if (overlap(outs[i], p, bytes)) {
                fail(MG_ERR_ARG, "%s: an output array overlaps an input array", who);
                return false;
            }
        for (size_t j = i + 1; j < outs.size(); ++j)
            if (overlap(outs[i], outs[j], bytes)) {
                fail(MG_ERR_ARG, "%s: two output arrays overlap", who);
                return false;
            }
    }
    return true;
}

// a table of n NodeBatchItems in device memory for the length of a call (scratch pool; uploaded on st)
struct DeviceTable {
    NodeBatchItem *dev = nullptr;
    bool upload(hipStream_t st, const std::vector<NodeBatchItem> &host)
    {
        const size_t bytes = host.size() * sizeof(NodeBatchItem);
        dev = static_cast<NodeBatchItem *>(scratch_pool().get(bytes));
        return dev && MG_HIP(hipMemcpyAsync(dev, host.data(), bytes, hipMemcpyHostToDevice, st));
    }
    ~DeviceTable()
    {
        if (dev) scratch_pool().put(dev);
    }
};

}  // namespace

extern "C" {

void mg_coefficientGradient(int N, double L, const double *lam, const double *U, double *gA)
{
    if (!require_ready("mg_coefficientGradient") || !shape_ok("mg_coefficientGradient", N, L)) return;
    if (!lam || !U || !gA || !aligned(lam) || !aligned(U) || !aligned(gA)) {
        fail(MG_ERR_ARG, "mg_coefficientGradient: a NULL or not 16-byte aligned array");
        return;
    }
    if (!no_overlap("mg_coefficientGradient", N, {Arrays{nullptr, nullptr, U, const_cast<double *>(lam), gA, nullptr}}, false)) return;
    {
        ProfScope ps("coef_grad", N, grad_bytes(N));
        k::coef_grad(ctx().stream, N, 0.5 * level0_inv(N, L), lam, U, gA);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_boundaryGradient(int N, double L, const double *a_dev, const double *lam, const double *Ubar, double *gU)
{
    if (!require_ready("mg_boundaryGradient") || !shape_ok("mg_boundaryGradient", N, L)) return;
    if (!lam || !gU || !aligned(lam) || !aligned(gU) || !aligned(a_dev) || !aligned(Ubar)) {
        fail(MG_ERR_ARG, "mg_boundaryGradient: a NULL lam or gU, or an array that is not 16-byte aligned");
        return;
    }
    if (!no_overlap("mg_boundaryGradient", N, {Arrays{a_dev, Ubar, nullptr, const_cast<double *>(lam), nullptr, gU}}, false)) return;
    {
        ProfScope ps("rim_grad", N, rim_bytes(N));
        k::rim_grad(ctx().stream, N, level0_inv(N, L), a_dev, lam, Ubar, gU);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_coefficientGradient_batch(int n, int N, double L, const double *const *lam, const double *const *U, double *const *gA)
{
    const char *who = "mg_coefficientGradient_batch";
    if (!require_ready(who) || !shape_ok(who, N, L)) return;
    if (n < 1 || n > 65535 || !lam || !U || !gA) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, 65535] or a NULL pointer array", who, n);
        return;
    }
    std::vector<Arrays> x(n);
    std::vector<NodeBatchItem> tab(n);
    for (int i = 0; i < n; ++i) {
        if (!lam[i] || !U[i] || !gA[i] || !aligned(lam[i]) || !aligned(U[i]) || !aligned(gA[i])) {
            fail(MG_ERR_ARG, "%s: a NULL or not 16-byte aligned array of instance %d", who, i);
            return;
        }
        x[i] = Arrays{nullptr, nullptr, U[i], const_cast<double *>(lam[i]), gA[i], nullptr};
        tab[i] = NodeBatchItem{lam[i], U[i], nullptr, gA[i], nullptr};
    }
    if (!no_overlap(who, N, x, false)) return;
    const hipStream_t st = ctx().stream;
    DeviceTable t;
    if (!t.upload(st, tab)) return;
    {
        ProfScope ps("coef_grad_batch", N, grad_bytes(N) * n);
        k::coef_grad_batch(st, n, N, 0.5 * level0_inv(N, L), t.dev);
    }
    (void)MG_HIP(hipStreamSynchronize(st));
}

void mg_boundaryGradient_batch(int n, int N, double L, const double *const *a_dev, const double *const *lam,
                               const double *const *Ubar, double *const *gU)
{
    const char *who = "mg_boundaryGradient_batch";
    if (!require_ready(who) || !shape_ok(who, N, L)) return;
    if (n < 1 || n > 65535 || !lam || !gU) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, 65535] or a NULL pointer array", who, n);
        return;
    }
    std::vector<Arrays> x(n);
    std::vector<NodeBatchItem> tab(n);
    for (int i = 0; i < n; ++i) {
        const double *a = a_dev ? a_dev[i] : nullptr, *ub = Ubar ? Ubar[i] : nullptr;
        if (!lam[i] || !gU[i] || !aligned(lam[i]) || !aligned(gU[i]) || !aligned(a) || !aligned(ub)) {
            fail(MG_ERR_ARG, "%s: a NULL lam or gU, or an array that is not 16-byte aligned, of instance %d", who, i);
            return;
        }
        x[i] = Arrays{a, ub, nullptr, const_cast<double *>(lam[i]), nullptr, gU[i]};
        tab[i] = NodeBatchItem{lam[i], ub, a, gU[i], nullptr};
    }
    if (!no_overlap(who, N, x, false)) return;
    const hipStream_t st = ctx().stream;
    DeviceTable t;
    if (!t.upload(st, tab)) return;
    {
        ProfScope ps("rim_grad_batch", N, rim_bytes(N) * n);
        k::rim_grad_batch(st, n, N, level0_inv(N, L), t.dev);
    }
    (void)MG_HIP(hipStreamSynchronize(st));
}

int mg_solver_adjoint(mg_solver *s, const double *Ubar, const double *U, double *lam, double *gA, double *gU, mg_solve_result *out)
{
    auto refuse = [&](int code) {
        if (out) {
            std::memset(out, 0, sizeof *out);
            out->status = code;
        }
        return code;
    };
    if (!require_ready("mg_solver_adjoint")) return refuse(MG_ERR_NOT_INIT);
    if (!s || !Ubar || !lam || (gA && !U)) {
        fail(MG_ERR_ARG, "mg_solver_adjoint: NULL solver, Ubar or lam, or gA wanted without U");
        return refuse(MG_ERR_ARG);
    }
    if (!aligned(Ubar) || !aligned(U) || !aligned(lam) || !aligned(gA) || !aligned(gU)) {
        fail(MG_ERR_ARG, "mg_solver_adjoint: every array must be 16-byte aligned");
        return refuse(MG_ERR_ARG);
    }
    if (solver_boundary(s)) {   // (include/mg_bc.h: the gradient kernels treat the whole rim as data)
        fail(MG_ERR_UNSUPPORTED, "mg_solver_adjoint: a boundary with a Neumann side is set; the adjoint is not built for boundary kinds");
        return refuse(MG_ERR_UNSUPPORTED);
    }
    if (mg_solver_has_reaction(s)) {   // (include/mg_reaction.h: no gradient in s is built, the rest is not offered without it)
        fail(MG_ERR_UNSUPPORTED, "mg_solver_adjoint: a reaction term is set; the adjoint is not built for a reaction here (mg_solver_adjoint_reaction takes it)");
        return refuse(MG_ERR_UNSUPPORTED);
    }
    double L = 1.0;
    const int N = solver_size(s, &L);
    const double *coef = solver_coefficient(s);   // (the solver's own level-0 array: what the solve itself reads)
    if (!no_overlap("mg_solver_adjoint", N, {Arrays{gU ? coef : nullptr, Ubar, gA ? U : nullptr, lam, gA, gU}}, true))
        return refuse(MG_ERR_ARG);
    const hipStream_t st = ctx().stream;
    if (!MG_HIP(hipMemsetAsync(lam, 0, (size_t)N * N * sizeof(double), st))) return refuse(MG_ERR_HIP);   // mg_fill_zero
    const int status = mg_solver_solve(s, Ubar, lam, out);
    if (status > 0) return status;
    if (!gA && !gU) return status;   // (just the solve, which has synchronised)
    const double inv = level0_inv(N, L);
    if (gA) {
        ProfScope ps("coef_grad", N, grad_bytes(N));
        k::coef_grad(st, N, 0.5 * inv, lam, U, gA);
    }
    if (gU) {
        ProfScope ps("rim_grad", N, rim_bytes(N));
        k::rim_grad(st, N, inv, coef, lam, Ubar, gU);
    }
    if (!MG_HIP(hipStreamSynchronize(st))) {
        if (out) out->status = MG_ERR_HIP;
        return MG_ERR_HIP;
    }
    return status;
}

int mg_batch_solver_adjoint(mg_batch_solver *s, int n, const double *const *Ubar, const double *const *U, double *const *lam,
                            double *const *gA, double *const *gU, mg_solve_result *out, mg_batch_solve_stats *stats)
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
    const char *who = "mg_batch_solver_adjoint";
    if (!require_ready(who)) return refuse(MG_ERR_NOT_INIT);
    if (!s || !Ubar || !lam || !out || (gA && !U)) {
        fail(MG_ERR_ARG, "%s: NULL solver, Ubar, lam or result array, or gA wanted without U", who);
        return refuse(MG_ERR_ARG);
    }
    N = batch_solver_size(s, &L, &max_batch);
    if (n < 1 || n > max_batch) {
        fail(MG_ERR_ARG, "%s: n = %d outside [1, max_batch = %d]", who, n, max_batch);
        return refuse(MG_ERR_ARG);
    }
    if (mg_batch_solver_has_reaction(s)) {   // (include/mg_rx_batch.h: refused as mg_solver_adjoint refuses it)
        fail(MG_ERR_UNSUPPORTED, "%s: a reaction term is set; the adjoint is not built for a reaction here (mg_batch_solver_adjoint_reaction takes it)", who);
        return refuse(MG_ERR_UNSUPPORTED);
    }
    const int n_coef = mg_batch_solver_has_coefficient(s);
    if (n_coef > 1 && n > n_coef) {
        fail(MG_ERR_ARG, "%s: n = %d instances, but the solver holds %d coefficients (one per instance)", who, n, n_coef);
        return refuse(MG_ERR_ARG);
    }
    std::vector<Arrays> x(n);
    std::vector<NodeBatchItem> tab((size_t)2 * n);   // [0, n): the coefficient gradient; [n, 2n): the rim gradient
    for (int i = 0; i < n; ++i) {
        const double *u = gA ? U[i] : nullptr, *coef = batch_solver_coefficient(s, i);
        double *ga = gA ? gA[i] : nullptr, *gu = gU ? gU[i] : nullptr;
        if (!Ubar[i] || !lam[i] || (gA && (!u || !ga)) || (gU && !gu)) {
            fail(MG_ERR_ARG, "%s: a NULL array of instance %d", who, i);
            return refuse(MG_ERR_ARG);
        }
        if (!aligned(Ubar[i]) || !aligned(lam[i]) || !aligned(u) || !aligned(ga) || !aligned(gu)) {
            fail(MG_ERR_ARG, "%s: every array of instance %d must be 16-byte aligned", who, i);
            return refuse(MG_ERR_ARG);
        }
        x[i] = Arrays{gU ? coef : nullptr, Ubar[i], u, lam[i], ga, gu};
        tab[i] = NodeBatchItem{lam[i], u, nullptr, ga, nullptr};
        tab[(size_t)n + i] = NodeBatchItem{lam[i], Ubar[i], coef, gu, nullptr};
    }
    if (!no_overlap(who, N, x, true)) return refuse(MG_ERR_ARG);
    const hipStream_t st = ctx().stream;
    DeviceTable t;
    if ((gA || gU) && !t.upload(st, tab)) return refuse(MG_ERR_HIP);
    for (int i = 0; i < n; ++i)
        if (!MG_HIP(hipMemsetAsync(lam[i], 0, (size_t)N * N * sizeof(double), st))) return refuse(MG_ERR_HIP);
    mg_batch_solve_stats bs;
    std::memset(&bs, 0, sizeof bs);
    const int status = mg_batch_solver_solve(s, n, Ubar, lam, out, &bs);
    if (status <= 0 && (gA || gU)) {
        const double inv = level0_inv(N, L);
        if (gA) {
            ProfScope ps("coef_grad_batch", N, grad_bytes(N) * n);
            k::coef_grad_batch(st, n, N, 0.5 * inv, t.dev);
            bs.launches += 1;
        }
        if (gU) {
            ProfScope ps("rim_grad_batch", N, rim_bytes(N) * n);
            k::rim_grad_batch(st, n, N, inv, t.dev + n);
            bs.launches += 1;
        }
        if (!MG_HIP(hipStreamSynchronize(st))) {
            for (int i = 0; i < n; ++i) out[i].status = MG_ERR_HIP;
            if (stats) *stats = bs;
            return MG_ERR_HIP;
        }
    }
    if (stats) *stats = bs;
    return status;
}

}  // extern "C"
