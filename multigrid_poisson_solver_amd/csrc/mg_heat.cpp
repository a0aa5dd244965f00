// mg_heat.cpp -- theta-scheme time stepping of the heat equation over the residual-tolerance solvers (include/mg_heat.h):
// one step is ONE launch of the right-hand-side kernel over the n instances (mg_heat_kernels.hip), then the inner solve with
// shift = sigma started from U itself.  A thin driver over mg_solver_solve / mg_batch_solver_solve: it owns the right-hand-side
// arrays and the table of the batched launch, a step allocates nothing and the host does not synchronise between the
// right-hand side and the solve.
// With a coefficient (include/mg_heat_vc.h, max_batch == 1 only) the inner mg_solver holds it; for theta != 1 the step's
// right-hand-side launch is k::heat_rhs_vc (mg_heat_vc_kernels.hip) on the solver's own level-0 array.
#include <cmath>
#include <cstring>
#include <vector>

#include "mg_internal.h"

using namespace mg;

struct mg_heat_stepper {
    int N = 0;
    double L = 1.0;
    int max_batch = 0;
    mg_heat_opts o{};
    double sigma = 0.0;
    k::HeatConsts hc;
    size_t pitch = 0;                        // doubles from one instance's F to the next one's (the batch solver's 256-byte pitch)
    double *F = nullptr;                     // max_batch right-hand sides
    NodeBatchItem *dev_tab = nullptr, *host_tab = nullptr;   // [max_batch]: in = U, coarse = Q, out = F (device / pinned)
    mg_solver *single = nullptr;             // max_batch == 1
    mg_batch_solver *batch = nullptr;        // max_batch > 1
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    std::vector<const double *> Fp;          // the F of every instance, as the batch solver takes them
    std::vector<mg_solve_result> res;
    std::vector<std::vector<int>> cycles;    // per instance: the cycles of every step of the last call
};

namespace {

bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }

// the scheme's parameters; false (after fail) when one is outside what the header allows
bool scheme_ok(const char *who, double nu, double dt, double theta)
{
    if (!finite_positive(nu) || !finite_positive(dt)) {
        fail(MG_ERR_ARG, "%s: nu = %g and dt = %g must be positive and finite", who, nu, dt);
        return false;
    }
    if (!(theta >= 0.5 && theta <= 1.0)) {
        fail(MG_ERR_ARG, "%s: theta = %g outside [0.5, 1]", who, theta);
        return false;
    }
    return true;
}

// the host constants of include/mg_heat.h, each operation rounded once and in its order; inv: level 0's of the solvers
k::HeatConsts heat_consts(int N, double L, double nu, double dt, double theta)
{
    mg_solve_opts so;
    mg_solve_opts_default(&so);
    k::HeatConsts c;
    const double a = theta * nu;
    c.sigma = 1.0 / (a * dt);
    c.beta = (1.0 - theta) / theta;
    c.gamma = 1.0 / a;
    c.inv = solve_level_consts(std::vector<int>{N}, L, so)[0].inv;
    c.lap = theta != 1.0;
    return c;
}

double rhs_bytes(int N, bool has_q) { return (double)N * N * (has_q ? 24.0 : 16.0); }
// with a coefficient (theta != 1): a is one more array read
double rhs_vc_bytes(int N, bool has_q) { return (double)N * N * (has_q ? 32.0 : 24.0); }

bool overlap(const void *a, const void *b, size_t bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

void release(mg_heat_stepper *s)
{
    if (s->single) mg_solver_destroy(s->single);
    if (s->batch) mg_batch_solver_destroy(s->batch);
    if (s->F) (void)hipFree(s->F);
    if (s->dev_tab) (void)hipFree(s->dev_tab);
    if (s->host_tab) (void)hipHostFree(s->host_tab);
    if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
    if (s->ev_end) (void)hipEventDestroy(s->ev_end);
    delete s;
}

}  // namespace

extern "C" {

void mg_heat_opts_default(mg_heat_opts *o)
{
    if (!o) return;
    o->nu = 1.0;
    o->dt = 1.0;
    o->theta = 1.0;
    mg_solve_opts_default(&o->solve);
}

void mg_heat_rhs(int N, double L, double nu, double dt, double theta, const double *U, const double *Q, double *F)
{
    if (!require_ready("mg_heat_rhs")) return;
    if (N < 3 || !finite_positive(L) || !U || !F) {
        fail(MG_ERR_ARG, "mg_heat_rhs: N = %d (at least 3), L = %g (positive, finite) or a NULL array", N, L);
        return;
    }
    if (!scheme_ok("mg_heat_rhs", nu, dt, theta)) return;
    if (((uintptr_t)U | (uintptr_t)Q | (uintptr_t)F) % 16 != 0) {
        fail(MG_ERR_ARG, "mg_heat_rhs: U, Q and F must be 16-byte aligned");
        return;
    }
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (overlap(F, U, bytes) || (Q && overlap(F, Q, bytes))) {
        fail(MG_ERR_ARG, "mg_heat_rhs: F overlaps U or Q");
        return;
    }
    const k::HeatConsts c = heat_consts(N, L, nu, dt, theta);
    {
        ProfScope ps(c.lap ? "heat_rhs<lap>" : "heat_rhs", N, rhs_bytes(N, Q != nullptr));
        k::heat_rhs(ctx().stream, N, c, U, Q, F);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

void mg_heat_rhs_coef(int N, double L, double nu, double dt, double theta, const double *a_dev, const double *U, const double *Q,
                      double *F)
{
    if (!require_ready("mg_heat_rhs_coef")) return;
    if (N < 3 || !finite_positive(L) || !U || !F) {
        fail(MG_ERR_ARG, "mg_heat_rhs_coef: N = %d (at least 3), L = %g (positive, finite) or a NULL array", N, L);
        return;
    }
    if (!scheme_ok("mg_heat_rhs_coef", nu, dt, theta)) return;
    if (((uintptr_t)a_dev | (uintptr_t)U | (uintptr_t)Q | (uintptr_t)F) % 16 != 0) {
        fail(MG_ERR_ARG, "mg_heat_rhs_coef: a, U, Q and F must be 16-byte aligned");
        return;
    }
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (overlap(F, U, bytes) || (Q && overlap(F, Q, bytes)) || (a_dev && overlap(F, a_dev, bytes))) {
        fail(MG_ERR_ARG, "mg_heat_rhs_coef: F overlaps a, U or Q");
        return;
    }
    const k::HeatConsts c = heat_consts(N, L, nu, dt, theta);
    if (a_dev && c.lap) {
        ProfScope ps("heat_rhs_vc", N, rhs_vc_bytes(N, Q != nullptr));
        k::heat_rhs_vc(ctx().stream, N, c, a_dev, U, Q, F);
    } else {   // a == 1, or theta == 1 (a is not read): mg_heat_rhs's launch
        ProfScope ps(c.lap ? "heat_rhs<lap>" : "heat_rhs", N, rhs_bytes(N, Q != nullptr));
        k::heat_rhs(ctx().stream, N, c, U, Q, F);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

mg_heat_stepper *mg_heat_stepper_create(int N, double L, int max_batch, const mg_heat_opts *opts)
{
    if (!require_ready("mg_heat_stepper_create")) return nullptr;
    mg_heat_opts o;
    mg_heat_opts_default(&o);
    if (opts) o = *opts;
    if (!scheme_ok("mg_heat_stepper_create", o.nu, o.dt, o.theta)) return nullptr;
    if (o.solve.shift != 0.0) {   // (also a NaN; the stepper sets the shift: an option is never silently overridden)
        fail(MG_ERR_ARG, "mg_heat_stepper_create: solve.shift = %g must be 0 (the stepper sets it to sigma = 1/(theta*nu*dt))",
             o.solve.shift);
        return nullptr;
    }
    if (max_batch < 1) {
        fail(MG_ERR_ARG, "mg_heat_stepper_create: max_batch = %d < 1", max_batch);
        return nullptr;
    }
    if (!solve_opts_ok("mg_heat_stepper_create", N, L, o.solve)) return nullptr;   // (N and L before the constants are formed)
    mg_heat_stepper *s = new mg_heat_stepper;
    s->N = N;
    s->L = L;
    s->max_batch = max_batch;
    s->o = o;
    s->hc = heat_consts(N, L, o.nu, o.dt, o.theta);
    s->sigma = s->hc.sigma;
    mg_solve_opts so = o.solve;
    so.shift = s->sigma;   // (an overflowing 1/(theta*nu*dt) is refused by the solver: shift must be finite)
    if (max_batch == 1) s->single = mg_solver_create(N, L, &so);
    else s->batch = mg_batch_solver_create(N, L, max_batch, &so);
    if (!s->single && !s->batch) {   // (the inner solver's refusal, its code and text, is the stepper's)
        release(s);
        return nullptr;
    }
    s->pitch = ((size_t)N * N + 31) / 32 * 32;
    const size_t tab_bytes = (size_t)max_batch * sizeof(NodeBatchItem), f_bytes = s->pitch * max_batch * sizeof(double);
    bool ok = MG_HIP(hipMalloc((void **)&s->F, f_bytes)) && MG_HIP(hipMalloc((void **)&s->dev_tab, tab_bytes)) &&
              MG_HIP(hipHostMalloc((void **)&s->host_tab, tab_bytes, hipHostMallocDefault)) &&
              MG_HIP(hipEventCreate(&s->ev_begin)) && MG_HIP(hipEventCreate(&s->ev_end));
    if (ok && pool_poison_wanted()) {   // MG_POOL_POISON: F does not start from what hipMalloc happened to return
        poison_block(s->F, f_bytes);
        ok = MG_HIP(hipStreamSynchronize(ctx().stream));
    }
    if (!ok) {
        release(s);
        return nullptr;
    }
    std::memset(s->host_tab, 0, tab_bytes);
    s->Fp.resize(max_batch);
    for (int i = 0; i < max_batch; ++i) s->Fp[i] = s->F + (size_t)i * s->pitch;
    s->res.resize(max_batch);
    s->cycles.resize(max_batch);
    return s;
}

int mg_heat_stepper_step(mg_heat_stepper *s, int n, double *const *U_dev, const double *const *Q_dev, int steps,
                         mg_heat_result *out)
{
    std::vector<mg_heat_result> r(n > 0 ? (size_t)n : 0);
    for (auto &x : r) std::memset(&x, 0, sizeof x);
    double device_ms = 0.0;
    auto finish = [&](int status) {
        if (out && s && n >= 1 && n <= s->max_batch) {
            for (int i = 0; i < n; ++i) {
                if (status > 0) r[i].status = status;
                r[i].device_ms = device_ms;
                r[i].n_steps = (int)s->cycles[i].size();
                r[i].cycles_per_step = s->cycles[i].empty() ? nullptr : s->cycles[i].data();
                out[i] = r[i];
            }
        }
        return status;
    };
    if (!require_ready("mg_heat_stepper_step")) return finish(MG_ERR_NOT_INIT);
    if (!s || !U_dev || !out) {
        fail(MG_ERR_ARG, "mg_heat_stepper_step: NULL stepper, array or result array");
        return finish(MG_ERR_ARG);
    }
    if (n < 1 || n > s->max_batch) {
        fail(MG_ERR_ARG, "mg_heat_stepper_step: n = %d outside [1, max_batch = %d]", n, s->max_batch);
        return finish(MG_ERR_ARG);
    }
    for (int i = 0; i < n; ++i) s->cycles[i].clear();
    if (steps < 1) {
        fail(MG_ERR_ARG, "mg_heat_stepper_step: steps = %d < 1", steps);
        return finish(MG_ERR_ARG);
    }
    const size_t bytes = (size_t)s->N * s->N * sizeof(double);
    for (int i = 0; i < n; ++i) {
        const double *Q = Q_dev ? Q_dev[i] : nullptr;
        if (!U_dev[i]) {
            fail(MG_ERR_ARG, "mg_heat_stepper_step: NULL U of instance %d", i);
            return finish(MG_ERR_ARG);
        }
        if (((uintptr_t)U_dev[i] | (uintptr_t)Q) % 16 != 0) {
            fail(MG_ERR_ARG, "mg_heat_stepper_step: U and Q of instance %d must be 16-byte aligned", i);
            return finish(MG_ERR_ARG);
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (j > i && overlap(U_dev[i], U_dev[j], bytes)) {
                fail(MG_ERR_ARG, "mg_heat_stepper_step: U of instances %d and %d overlap", i, j);
                return finish(MG_ERR_ARG);
            }
            if (Q_dev && Q_dev[j] && overlap(U_dev[i], Q_dev[j], bytes)) {
                fail(MG_ERR_ARG, "mg_heat_stepper_step: U of instance %d overlaps Q of instance %d", i, j);
                return finish(MG_ERR_ARG);
            }
        }
    const hipStream_t st = ctx().stream;
    bool any_q = false;
    for (int i = 0; i < n; ++i) {
        const double *Q = Q_dev ? Q_dev[i] : nullptr;
        any_q = any_q || Q;
        s->host_tab[i] = NodeBatchItem{U_dev[i], nullptr, Q, s->F + (size_t)i * s->pitch, nullptr};
        s->cycles[i].reserve((size_t)steps);
    }
    if (!MG_HIP(hipEventRecord(s->ev_begin, st))) return finish(MG_ERR_HIP);
    if (!MG_HIP(hipMemcpyAsync(s->dev_tab, s->host_tab, (size_t)n * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)))
        return finish(MG_ERR_HIP);
    int status = MG_SOLVE_CONVERGED;
    // (max_batch == 1 with a coefficient and theta != 1: the variable right-hand side on the solver's level-0 coefficient)
    const double *coef = s->single && s->hc.lap ? solver_coefficient(s->single) : nullptr;
    // (include/mg_bc.h: with a boundary the right-hand side runs over the unknowns, whatever theta)
    const int *kind = s->single ? solver_boundary(s->single) : nullptr;
    for (int step = 0; step < steps && status == MG_SOLVE_CONVERGED; ++step) {
        if (kind) {
            ProfScope ps("heat_rhs_bc", s->N, s->hc.lap && solver_coefficient(s->single) ? rhs_vc_bytes(s->N, any_q) : rhs_bytes(s->N, any_q));
            k::heat_rhs_bc(st, s->N, s->hc, kind, solver_coefficient(s->single), U_dev[0], Q_dev ? Q_dev[0] : nullptr, s->F);
        } else if (coef) {
            ProfScope ps("heat_rhs_vc", s->N, rhs_vc_bytes(s->N, any_q));
            k::heat_rhs_vc(st, s->N, s->hc, coef, U_dev[0], Q_dev ? Q_dev[0] : nullptr, s->F);
        } else {
            ProfScope ps(s->hc.lap ? "heat_rhs<lap>" : "heat_rhs", s->N, rhs_bytes(s->N, any_q) * n);
            k::heat_rhs_batch(st, n, s->N, s->hc, s->dev_tab);
        }
        status = s->single ? mg_solver_solve(s->single, s->Fp[0], U_dev[0], &s->res[0])
                           : mg_batch_solver_solve(s->batch, n, s->Fp.data(), U_dev, s->res.data(), nullptr);
        if (status > 0) return finish(status);
        for (int i = 0; i < n; ++i) {
            const mg_solve_result &x = s->res[i];
            r[i].steps += 1;
            r[i].cycles += x.cycles;
            if (x.coarse_capped) r[i].coarse_capped = 1;
            r[i].res = x.res;
            r[i].ref_norm = x.ref_norm;
            r[i].status = x.status;
            s->cycles[i].push_back(x.cycles);
        }
    }
    if (!MG_HIP(hipEventRecord(s->ev_end, st)) || !MG_HIP(hipEventSynchronize(s->ev_end))) return finish(MG_ERR_HIP);
    float ms = 0.0f;
    if (MG_HIP(hipEventElapsedTime(&ms, s->ev_begin, s->ev_end))) device_ms = ms;
    return finish(status);
}

double mg_heat_stepper_sigma(const mg_heat_stepper *s) { return s ? s->sigma : 0.0; }

// ------------------------------------------------------------------ variable coefficient (include/mg_heat_vc.h)
int mg_heat_stepper_set_coefficient(mg_heat_stepper *s, const double *a_dev)
{
    if (!require_ready("mg_heat_stepper_set_coefficient")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_heat_stepper_set_coefficient: NULL stepper");
        return MG_ERR_ARG;
    }
    if (!s->single) {
        if (!a_dev) return MG_OK;   // (a batched stepper never has one)
        fail(MG_ERR_UNSUPPORTED, "mg_heat_stepper_set_coefficient: the stepper was created with max_batch = %d; the batched "
                                 "solver has no variable coefficient", s->max_batch);
        return MG_ERR_UNSUPPORTED;
    }
    // the solver checks, copies and coarsens; its refusal -- code and text -- is the stepper's, and leaves both as they were
    return mg_solver_set_coefficient(s->single, a_dev);
}

int mg_heat_stepper_has_coefficient(const mg_heat_stepper *s) { return s && s->single ? mg_solver_has_coefficient(s->single) : 0; }

// ------------------------------------------------------------------ boundary kinds per side (include/mg_bc.h)
void mg_heat_rhs_boundary(int N, double L, double nu, double dt, double theta, const int *kind, const double *a_dev,
                          const double *U, const double *Q, double *F)
{
    if (!require_ready("mg_heat_rhs_boundary")) return;
    if (N < 3 || !finite_positive(L) || !U || !F) {
        fail(MG_ERR_ARG, "mg_heat_rhs_boundary: N = %d (at least 3), L = %g (positive, finite) or a NULL array", N, L);
        return;
    }
    if (!scheme_ok("mg_heat_rhs_boundary", nu, dt, theta)) return;
    if (!kind || ((kind[0] | kind[1] | kind[2] | kind[3]) & ~1) != 0) {
        fail(MG_ERR_ARG, "mg_heat_rhs_boundary: kind must be a host int[4] of MG_BC_DIRICHLET (0) / MG_BC_NEUMANN (1)");
        return;
    }
    if (((uintptr_t)a_dev | (uintptr_t)U | (uintptr_t)Q | (uintptr_t)F) % 16 != 0) {
        fail(MG_ERR_ARG, "mg_heat_rhs_boundary: a, U, Q and F must be 16-byte aligned");
        return;
    }
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (overlap(F, U, bytes) || (Q && overlap(F, Q, bytes)) || (a_dev && overlap(F, a_dev, bytes))) {
        fail(MG_ERR_ARG, "mg_heat_rhs_boundary: F overlaps a, U or Q");
        return;
    }
    const k::HeatConsts c = heat_consts(N, L, nu, dt, theta);
    {
        ProfScope ps("heat_rhs_bc", N, a_dev && c.lap ? rhs_vc_bytes(N, Q != nullptr) : rhs_bytes(N, Q != nullptr));
        k::heat_rhs_bc(ctx().stream, N, c, kind, a_dev, U, Q, F);
    }
    (void)MG_HIP(hipStreamSynchronize(ctx().stream));
}

int mg_heat_stepper_set_boundary(mg_heat_stepper *s, const int *kind)
{
    if (!require_ready("mg_heat_stepper_set_boundary")) return MG_ERR_NOT_INIT;
    if (!s) {
        fail(MG_ERR_ARG, "mg_heat_stepper_set_boundary: NULL stepper");
        return MG_ERR_ARG;
    }
    if (!s->single) {
        if (kind && ((kind[0] | kind[1] | kind[2] | kind[3]) == 0)) return MG_OK;   // (a batched stepper never has one)
        if (!kind) {
            fail(MG_ERR_ARG, "mg_heat_stepper_set_boundary: NULL kind (a host int[4]: S, N, W, E)");
            return MG_ERR_ARG;
        }
        fail(MG_ERR_UNSUPPORTED, "mg_heat_stepper_set_boundary: the stepper was created with max_batch = %d; the batched solver "
                                 "has no boundary kinds", s->max_batch);
        return MG_ERR_UNSUPPORTED;
    }
    // the solver checks and keeps the kinds; its refusal -- code and text -- is the stepper's, and leaves both as they were
    return mg_solver_set_boundary(s->single, kind);
}

void mg_heat_stepper_destroy(mg_heat_stepper *s)
{
    if (!s) return;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    release(s);
}

}  // extern "C"
