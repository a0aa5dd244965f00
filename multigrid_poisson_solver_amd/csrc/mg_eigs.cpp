// mg_eigs.cpp -- the lowest eigenmodes of -div(a grad u): multigrid-preconditioned LOBPCG (include/mg_eigs.h is the
// specification).  The driver owns the 6p basis fields S = [X, W, P], AS and the small tables; the preconditioner and the
// operator are the batch solver's own launches over the p columns -- an internal mg_batch_solver for p instances whose cycle
// is entered through mg::batch_solver_cycle (mg_solve_batch.cpp) and mg_applyOperator's batched launch with the constant
// -inv --, so a solve enqueues nothing per column.  The Gram matrices, the rotation and the recomputed residual are the
// kernels of mg_eigs_kernels.hip; the Rayleigh-Ritz step between them runs on the host (mg_eigs_rr.h) on 2 m^2 doubles read
// back once per step.
#include <cmath>
#include <cstring>
#include <vector>

#include "mg_eigs_rr.h"
#include "mg_internal.h"

using namespace mg;

struct mg_eigs {
    int N = 0, p = 0;
    double L = 1.0, neg_inv = 0.0;
    mg_eigs_opts o{};
    mg_batch_solver *bs = nullptr;
    size_t pitch = 0;                        // doubles from one field to the next (N^2 rounded up to 32)
    double *fields = nullptr;                // 6p fields: S[0 .. 3p) then AS[0 .. 3p)
    double *S[k::EIGS_MAX_M] = {}, *AS[k::EIGS_MAX_M] = {};
    double *gram_part = nullptr, *gram_out = nullptr, *rot_part = nullptr, *res2 = nullptr, *coef = nullptr;
    double **ptrs = nullptr;                 // device: EIGS_PTR_COUNT pointers (the rotation's layout; the Gram tables follow)
    double **gram_ptrs = nullptr;            // device: per basis size m = p, 2p, 3p the 2m pointers S then AS
    NodeBatchItem *apply_tab = nullptr;      // device: [0, p) X -> AX, [p, 2p) W -> AW
    void *pinned = nullptr;                  // one pinned block: gram read-back, res2, coef staging, the apply tables
    double *h_gram = nullptr, *h_res2 = nullptr, *h_coef = nullptr;
    NodeBatchItem *h_apply = nullptr;
    std::vector<double> history;             // 2k + 2 doubles per Rayleigh-Ritz step
    int records = 0;
};

namespace {

size_t gram_sums(int m) { return (size_t)k::eigs_tiles(m) * k::EIGS_TILE_SUMS; }

void release(mg_eigs *e)
{
    if (e->bs) mg_batch_solver_destroy(e->bs);
    for (void *q : {(void *)e->fields, (void *)e->gram_part, (void *)e->gram_out, (void *)e->rot_part, (void *)e->res2,
                    (void *)e->coef, (void *)e->ptrs, (void *)e->gram_ptrs, (void *)e->apply_tab})
        if (q) (void)hipFree(q);
    if (e->pinned) (void)hipHostFree(e->pinned);
    delete e;
}

// G, H (m x m) from the finished tile sums: entry (j, l), j <= l, of tile (j / T, l / T), mirrored
void gram_unpack(int m, const double *out, double *G, double *H)
{
    constexpr int T = k::EIGS_TILE;
    const int nt = (m + T - 1) / T;
    for (int j = 0; j < m; ++j)
        for (int l = j; l < m; ++l) {
            const int a = j / T, b = l / T;
            const int z = a * nt - a * (a - 1) / 2 + (b - a);   // row-major over a <= b
            const double *t = out + (size_t)z * k::EIGS_TILE_SUMS;
            const int e = (j % T) * T + l % T;
            G[(size_t)j * m + l] = G[(size_t)l * m + j] = t[e];
            H[(size_t)j * m + l] = H[(size_t)l * m + j] = t[T * T + e];
        }
}

// C, Cp (m x p row-major) and theta into the kernel's layout: columns of EIGS_MAX_M entries, padded with +0
void coef_pack(int m, int p, const double *C, const double *Cp, const double *theta, double *dst)
{
    std::memset(dst, 0, k::EIGS_COEF_COUNT * sizeof(double));
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j < m; ++j) {
            dst[i * k::EIGS_MAX_M + j] = C[(size_t)j * p + i];
            dst[k::EIGS_COEF_CP + i * k::EIGS_MAX_M + j] = Cp[(size_t)j * p + i];
        }
        dst[k::EIGS_COEF_THETA + i] = theta[i];
    }
}

bool overlap(const void *a, const void *b, size_t bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

bool sync(hipStream_t st) { return MG_HIP(hipStreamSynchronize(st)); }

}  // namespace

extern "C" {

void mg_eigs_opts_default(mg_eigs_opts *o)
{
    if (!o) return;
    mg_solve_opts_default(&o->cycle);
    o->k = 1;
    o->guard = 0;
    o->max_iters = 60;
    o->rtol = 1e-8;
    o->atol = 0.0;
}

mg_eigs *mg_eigs_create(int N, double L, const mg_eigs_opts *opts)
{
    if (!require_ready("mg_eigs_create")) return nullptr;
    mg_eigs_opts o;
    mg_eigs_opts_default(&o);
    if (opts) o = *opts;
    auto refuse = [](const char *what) {
        fail(MG_ERR_ARG, "mg_eigs_create: %s", what);
        return (mg_eigs *)nullptr;
    };
    if (o.cycle.shift != 0.0) return refuse("cycle.shift must be 0: the eigenvalues of the shifted operator are lambda + shift, add it to the result");
    if (o.cycle.fmg != 0) return refuse("cycle.fmg must be 0: the preconditioner is one V-cycle");
    if (o.k < 1) return refuse("k < 1");
    if (o.guard < 0) return refuse("guard < 0");
    if (o.k > MG_EIGS_MAX_BLOCK || o.guard > MG_EIGS_MAX_BLOCK || o.k + o.guard > MG_EIGS_MAX_BLOCK)
        return refuse("k + guard exceeds MG_EIGS_MAX_BLOCK (12)");
    if (o.max_iters < 0) return refuse("max_iters < 0");
    if (!(o.rtol >= 0.0) || !(o.rtol < HUGE_VAL) || !(o.atol >= 0.0) || !(o.atol < HUGE_VAL)) return refuse("rtol and atol must be finite and >= 0");
    {   // (the cycle's own stopping rule plays no part: the preconditioner is exactly one cycle)
        mg_solve_opts d;
        mg_solve_opts_default(&d);
        o.cycle.rtol = d.rtol;
        o.cycle.atol = d.atol;
        o.cycle.max_cycles = d.max_cycles;
    }
    if (!solve_opts_ok("mg_eigs_create", N, L, o.cycle)) return nullptr;
    const int p = o.k + o.guard;
    if (3.0 * p > ((double)N - 2.0) * ((double)N - 2.0)) return refuse("3(k + guard) exceeds the (N-2)^2 interior points");
    if (N < 2 * o.cycle.N_min) return refuse("N < 2*N_min: a hierarchy of one level has no cycle to precondition with");
    mg_eigs *e = new mg_eigs;
    e->N = N;
    e->L = L;
    e->p = p;
    e->o = o;
    e->bs = mg_batch_solver_create(N, L, p, &o.cycle);
    if (!e->bs) {
        release(e);
        return nullptr;
    }
    e->neg_inv = -solve_level_consts(std::vector<int>{N}, L, o.cycle)[0].inv;
    e->pitch = ((size_t)N * N + 31) / 32 * 32;
    const size_t n_fields = 6 * (size_t)p * e->pitch;
    const size_t n_gram_part = gram_sums(3 * p) * k::eigs_gram_blocks(N), n_rot_part = (size_t)p * k::eigs_rotate_blocks(N);
    const size_t n_gram_ptrs = 2 * (size_t)(p + 2 * p + 3 * p);
    const size_t pinned_doubles = gram_sums(3 * p) + MG_EIGS_MAX_BLOCK + k::EIGS_COEF_COUNT;
    const size_t pinned_bytes = pinned_doubles * sizeof(double) + 2 * (size_t)p * sizeof(NodeBatchItem);
    auto dalloc = [](double **q, size_t n) { return MG_HIP(hipMalloc((void **)q, n * sizeof(double))); };
    bool ok = dalloc(&e->fields, n_fields) && dalloc(&e->gram_part, n_gram_part) && dalloc(&e->gram_out, gram_sums(3 * p)) &&
              dalloc(&e->rot_part, n_rot_part) && dalloc(&e->res2, MG_EIGS_MAX_BLOCK) && dalloc(&e->coef, k::EIGS_COEF_COUNT) &&
              MG_HIP(hipMalloc((void **)&e->ptrs, k::EIGS_PTR_COUNT * sizeof(double *))) &&
              MG_HIP(hipMalloc((void **)&e->gram_ptrs, n_gram_ptrs * sizeof(double *))) &&
              MG_HIP(hipMalloc((void **)&e->apply_tab, 2 * (size_t)p * sizeof(NodeBatchItem))) &&
              MG_HIP(hipHostMalloc(&e->pinned, pinned_bytes, hipHostMallocDefault));
    if (ok) {
        for (int j = 0; j < 3 * p; ++j) {
            e->S[j] = e->fields + (size_t)j * e->pitch;
            e->AS[j] = e->fields + (size_t)(3 * p + j) * e->pitch;
        }
        // the tables never change: the rotation's (S, AS, R = the fields of AW) and the Gram kernel's per basis size
        std::vector<double *> t(k::EIGS_PTR_COUNT, nullptr), g;
        for (int j = 0; j < 3 * p; ++j) {
            t[j] = e->S[j];
            t[k::EIGS_PTR_AS + j] = e->AS[j];
        }
        for (int i = 0; i < p; ++i) t[k::EIGS_PTR_R + i] = e->AS[p + i];
        for (int m = p; m <= 3 * p; m += p) {
            for (int j = 0; j < m; ++j) g.push_back(e->S[j]);
            for (int j = 0; j < m; ++j) g.push_back(e->AS[j]);
        }
        e->h_gram = static_cast<double *>(e->pinned);
        e->h_res2 = e->h_gram + gram_sums(3 * p);
        e->h_coef = e->h_res2 + MG_EIGS_MAX_BLOCK;
        e->h_apply = reinterpret_cast<NodeBatchItem *>(e->h_coef + k::EIGS_COEF_COUNT);
        // (the rim of every field is +0 from here on: no kernel of a solve writes it again but the operator, which writes +0)
        ok = MG_HIP(hipMemcpy(e->ptrs, t.data(), t.size() * sizeof(double *), hipMemcpyHostToDevice)) &&
             MG_HIP(hipMemcpy(e->gram_ptrs, g.data(), g.size() * sizeof(double *), hipMemcpyHostToDevice)) &&
             MG_HIP(hipMemset(e->fields, 0, n_fields * sizeof(double))) && MG_HIP(hipMemset(e->res2, 0, MG_EIGS_MAX_BLOCK * sizeof(double)));
    }
    if (!ok) {
        release(e);
        return nullptr;
    }
    e->history.reserve((size_t)(o.max_iters + 1) * (2 * o.k + 2));
    return e;
}

int mg_eigs_set_coefficient(mg_eigs *e, const double *a_dev)
{
    if (!require_ready("mg_eigs_set_coefficient")) return MG_ERR_NOT_INIT;
    if (!e) {
        fail(MG_ERR_ARG, "mg_eigs_set_coefficient: NULL solver");
        return MG_ERR_ARG;
    }
    if (!a_dev) return mg_batch_solver_set_coefficient(e->bs, 0, nullptr);
    return mg_batch_solver_set_coefficient(e->bs, 1, &a_dev);
}

int mg_eigs_solve(mg_eigs *e, double *const *X_dev, int use_start, uint64_t seed, double *lam, double *res, mg_eigs_result *out)
{
    mg_eigs_result r;
    std::memset(&r, 0, sizeof r);
    auto finish = [&](int status) {
        r.status = status;
        if (out) *out = r;
        return status;
    };
    if (!require_ready("mg_eigs_solve")) return finish(MG_ERR_NOT_INIT);
    if (!e || !X_dev || !lam || !res || !out) {
        fail(MG_ERR_ARG, "mg_eigs_solve: NULL solver, array of vectors, lam, res or result");
        return finish(MG_ERR_ARG);
    }
    const int N = e->N, p = e->p, kk = e->o.k;
    const size_t n0 = (size_t)N * N, bytes = n0 * sizeof(double);
    for (int i = 0; i < kk; ++i) {
        if (!X_dev[i] || (uintptr_t)X_dev[i] % 16 != 0) {
            fail(MG_ERR_ARG, "mg_eigs_solve: vector %d is NULL or not 16-byte aligned", i);
            return finish(MG_ERR_ARG);
        }
        for (int j = 0; j < i; ++j)
            if (overlap(X_dev[i], X_dev[j], bytes)) {
                fail(MG_ERR_ARG, "mg_eigs_solve: vectors %d and %d overlap", j, i);
                return finish(MG_ERR_ARG);
            }
    }
    const hipStream_t st = ctx().stream;
    const double *a = batch_solver_coefficient(e->bs, 0);
    e->history.clear();
    e->records = 0;
    // the start, and the operator tables (the coefficient may have changed since the last solve)
    for (int i = 0; i < p; ++i) {
        if (use_start && i < kk) {
            k::eigs_start(st, N, e->S[i], X_dev[i]);
        } else {
            k::fill_uniform(st, e->S[i], n0, seed + (uint64_t)i);
            k::eigs_start(st, N, e->S[i], nullptr);
        }
        e->h_apply[i] = NodeBatchItem{e->S[i], nullptr, a, e->AS[i], nullptr};
        e->h_apply[p + i] = NodeBatchItem{e->S[p + i], nullptr, a, e->AS[p + i], nullptr};
    }
    if (!MG_HIP(hipMemcpyAsync(e->apply_tab, e->h_apply, 2 * (size_t)p * sizeof(NodeBatchItem), hipMemcpyHostToDevice, st)))
        return finish(MG_ERR_HIP);
    const double pts = (double)N * N, apply_bytes = pts * p * (a ? 24.0 : 16.0);
    auto apply_x = [&]() {
        ProfScope ps("eig_apply", N, apply_bytes);
        k::apply_vc_batch(st, p, N, e->neg_inv, 0.0, e->apply_tab);
    };
    std::vector<double> G((size_t)9 * p * p), H((size_t)9 * p * p), C((size_t)3 * p * p), Cp((size_t)3 * p * p), theta(p, 0.0), rr(p, 0.0);
    std::vector<const double *> F0(p);
    std::vector<double *> U0(p);
    for (int i = 0; i < p; ++i) {
        F0[i] = e->AS[p + i];   // R_i
        U0[i] = e->S[p + i];    // W_i
    }
    auto upload_theta = [&]() {
        for (int i = 0; i < p; ++i) e->h_coef[k::EIGS_COEF_THETA + i] = theta[i];
        return MG_HIP(hipMemcpyAsync(e->coef + k::EIGS_COEF_THETA, e->h_coef + k::EIGS_COEF_THETA, p * sizeof(double),
                                     hipMemcpyHostToDevice, st));
    };
    // R_i = AX_i - theta_i*X_i and res_i into rr, from the AX and the theta that are there; false on a HIP error
    auto residuals = [&]() {
        {
            ProfScope ps("eig_resnorm", N, pts * 24.0 * p);
            k::eigs_resnorm(st, N, p, e->ptrs, e->coef, e->rot_part, e->res2);
        }
        if (!MG_HIP(hipMemcpyAsync(e->h_res2, e->res2, p * sizeof(double), hipMemcpyDeviceToHost, st)) || !sync(st)) return false;
        for (int i = 0; i < p; ++i) rr[i] = std::sqrt(e->h_res2[i]);
        return true;
    };
    // everything that is reported, recomputed from X alone: AX = AA*X, theta_i = <x_i, AX_i>/<x_i, x_i> (the Gram launch on
    // [X]), R and res
    auto recompute = [&]() {
        apply_x();
        {
            ProfScope ps("eig_gram", N, pts * 16.0 * p);
            k::eigs_gram(st, N, p, e->gram_ptrs, e->gram_part, e->gram_out);
        }
        if (!MG_HIP(hipMemcpyAsync(e->h_gram, e->gram_out, gram_sums(p) * sizeof(double), hipMemcpyDeviceToHost, st)) || !sync(st))
            return false;
        gram_unpack(p, e->h_gram, G.data(), H.data());
        for (int i = 0; i < p; ++i) theta[i] = H[(size_t)i * p + i] / G[(size_t)i * p + i];
        return upload_theta() && residuals();
    };
    auto met = [&]() {
        for (int i = 0; i < kk; ++i)
            if (!(rr[i] <= std::fmax(e->o.rtol * theta[i], e->o.atol))) return false;
        return true;
    };
    apply_x();
    int m = p, it = 0, refills = 0;
    bool cycle_pending = false;
    std::vector<char> locked(p, 0), active((size_t)3 * p, 1);
    std::vector<double> prev_rr(p, HUGE_VAL);
    bool recomputed = false;   // rr holds recomputed residuals of the current X
    const double *const *gram_tab = nullptr;
    for (;;) {
        gram_tab = e->gram_ptrs + (m == p ? 0 : m == 2 * p ? 2 * p : 6 * p);
        {
            ProfScope ps("eig_gram", N, pts * 16.0 * m);
            k::eigs_gram(st, N, m, gram_tab, e->gram_part, e->gram_out);
        }
        if (!MG_HIP(hipMemcpyAsync(e->h_gram, e->gram_out, gram_sums(m) * sizeof(double), hipMemcpyDeviceToHost, st)) || !sync(st))
            return finish(MG_ERR_HIP);
        gram_unpack(m, e->h_gram, G.data(), H.data());
        if (cycle_pending) {   // (the read-back above synchronised behind the last cycle's state copy)
            if (batch_solver_coarse_capped(e->bs, p)) r.coarse_capped = 1;
            cycle_pending = false;
        }
        if (it == 0 && e->records == 0)   // (what a breakdown of the very first step reports: the Rayleigh quotients of the start)
            for (int i = 0; i < p; ++i) theta[i] = H[(size_t)i * m + i] / G[(size_t)i * m + i];
        if (use_start && it == 0 && e->records == 0 && refills == 0) {
            // a start that already IS a solution is returned untouched: its k columns orthonormal within the bound of their
            // Gram sums (4 n u/(1 - n u), n = (N-2)^2) and the residuals of their Rayleigh quotients inside the tolerance.
            // These are the launches of the recomputation above, so the values reported are the bits a solve that ended on
            // these vectors reported.
            const double n_pts = ((double)N - 2.0) * ((double)N - 2.0), u = std::ldexp(1.0, -53);
            const double orth = 4.0 * n_pts * u / (1.0 - n_pts * u);
            bool orthonormal = true;
            for (int i = 0; i < kk && orthonormal; ++i)
                for (int j = i; j < kk && orthonormal; ++j)
                    orthonormal = std::fabs(G[(size_t)i * m + j] - (i == j ? 1.0 : 0.0)) <= orth;
            if (orthonormal) {
                if (!upload_theta() || !residuals()) return finish(MG_ERR_HIP);
                if (met()) {
                    for (int i = 0; i < kk; ++i) e->history.push_back(theta[i]);
                    for (int i = 0; i < kk; ++i) e->history.push_back(rr[i]);
                    e->history.push_back((double)p);
                    e->history.push_back(0.0);
                    e->records += 1;
                    r.converged = 1;
                    recomputed = true;
                    break;
                }
            }
        }
        // soft locking: W_i and P_i of a locked column stay out of the basis (a cycle applied to rounding noise, and a
        // difference of nearly equal vectors: with them in, converged columns drift away again); the launches do not change
        for (int j = 0; j < m; ++j) active[j] = j < p || !locked[j % p];
        const int kept = eigs_rr::rayleigh_ritz_masked(m, p, MG_EIGS_DROP, active.data(), G.data(), H.data(), C.data(), Cp.data(),
                                                       theta.data());
        if (kept < p && it == 0 && e->records == 0 && refills < 3) {
            // a START of fewer than p independent columns (no W exists yet to refill the basis): the dependent columns -- those
            // a Cholesky sweep over the scaled Gram matrix, in column order, leaves with a squared residual <= 1e-9 -- are
            // replaced by random ones, and the step is taken again
            std::vector<double> Lc((size_t)p * p, 0.0);
            std::vector<char> dep(p, 0);
            for (int j = 0; j < p; ++j) {
                const double gj = G[(size_t)j * m + j];
                double r2 = 1.0;
                for (int i = 0; i < j; ++i) {
                    if (dep[i]) continue;
                    double v = G[(size_t)i * m + j] / std::sqrt(G[(size_t)i * m + i] * gj);
                    for (int t = 0; t < i; ++t)
                        if (!dep[t]) v -= Lc[(size_t)i * p + t] * Lc[(size_t)j * p + t];
                    v /= Lc[(size_t)i * p + i];
                    Lc[(size_t)j * p + i] = v;
                    r2 -= v * v;
                }
                dep[j] = !(gj > 0.0) || !(gj < HUGE_VAL) || !(r2 > 1e-9);
                Lc[(size_t)j * p + j] = dep[j] ? 1.0 : std::sqrt(r2);
            }
            ++refills;
            bool any = false;
            for (int j = 0; j < p; ++j)
                if (dep[j]) {
                    k::fill_uniform(st, e->S[j], n0, seed + (uint64_t)(refills * p + j));
                    k::eigs_start(st, N, e->S[j], nullptr);
                    any = true;
                }
            if (any) {
                apply_x();
                continue;
            }
        }
        if (kept < p) {
            r.breakdown = 1;
            e->history.insert(e->history.end(), (size_t)2 * kk, 0.0);
            e->history.push_back((double)kept);
            e->history.push_back(0.0);
            e->records += 1;
            break;
        }
        coef_pack(m, p, C.data(), Cp.data(), theta.data(), e->h_coef);
        if (!MG_HIP(hipMemcpyAsync(e->coef, e->h_coef, k::EIGS_COEF_COUNT * sizeof(double), hipMemcpyHostToDevice, st))) return finish(MG_ERR_HIP);
        {
            ProfScope ps("eig_rotate", N, pts * (16.0 * m + 40.0 * p));
            k::eigs_rotate(st, N, m, p, e->ptrs, e->coef, e->rot_part, e->res2);
        }
        if (!MG_HIP(hipMemcpyAsync(e->h_res2, e->res2, p * sizeof(double), hipMemcpyDeviceToHost, st)) || !sync(st)) return finish(MG_ERR_HIP);
        for (int i = 0; i < p; ++i) rr[i] = std::sqrt(e->h_res2[i]);
        recomputed = false;
        for (int i = 0; i < p; ++i) {   // locked: inside the tolerance and no longer decreasing; kept while inside it
            locked[i] = rr[i] <= std::fmax(e->o.rtol * theta[i], e->o.atol) && (locked[i] || rr[i] >= prev_rr[i]);
            prev_rr[i] = rr[i];
        }
        for (int i = 0; i < kk; ++i) e->history.push_back(theta[i]);
        for (int i = 0; i < kk; ++i) e->history.push_back(rr[i]);
        e->history.push_back((double)kept);
        e->history.push_back(0.0);
        e->records += 1;
        bool have_p = m > p;
        if (met()) {   // the rotated residual met the tolerance: the recomputed one decides
            if (!recompute()) return finish(MG_ERR_HIP);
            recomputed = true;
            if (met()) {
                r.converged = 1;
                break;
            }
            have_p = false;   // a RESTART
            r.restarts += 1;
            e->history.back() = 1.0;
        }
        if (it == e->o.max_iters) break;
        if (!MG_HIP(hipMemsetAsync(e->S[p], 0, (size_t)p * e->pitch * sizeof(double), st))) return finish(MG_ERR_HIP);
        {
            ProfScope ps("eig_cycle", N, 0.0);
            if (batch_solver_cycle(e->bs, st, p, F0.data(), U0.data()) < 0) return finish(MG_ERR_HIP);
            if (!batch_solver_enqueue_state(e->bs, st)) return finish(MG_ERR_HIP);
            cycle_pending = true;
        }
        {
            ProfScope ps("eig_apply", N, apply_bytes);
            k::apply_vc_batch(st, p, N, e->neg_inv, 0.0, e->apply_tab + p);
        }
        ++it;
        recomputed = false;
        m = have_p ? 3 * p : 2 * p;
    }
    if (!recomputed && !recompute()) return finish(MG_ERR_HIP);
    for (int i = 0; i < kk; ++i) {
        if (!MG_HIP(hipMemcpyAsync(X_dev[i], e->S[i], bytes, hipMemcpyDeviceToDevice, st))) return finish(MG_ERR_HIP);
        lam[i] = theta[i];
        res[i] = rr[i];
    }
    if (!sync(st)) return finish(MG_ERR_HIP);
    r.iters = it;
    r.cycles = p * it;
    return finish(r.converged ? MG_SOLVE_CONVERGED : MG_SOLVE_NOT_CONVERGED);
}

int mg_eigs_history(const mg_eigs *e, double *out, int cap)
{
    if (!e) return 0;
    if (!out) return e->records;
    const int n = cap < e->records ? (cap > 0 ? cap : 0) : e->records;
    if (n > 0) std::memcpy(out, e->history.data(), (size_t)n * (2 * e->o.k + 2) * sizeof(double));
    return n;
}

void mg_eigs_destroy(mg_eigs *e)
{
    if (!e) return;
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    release(e);
}

// ------------------------------------------------------------------ test hooks
int mg_eigsRayleighRitz(int m, int p, const double *G, const double *H, double *C, double *Cp, double *theta)
{
    if (m < 1 || m > k::EIGS_MAX_M || p < 1 || p > m || !G || !H || !C || !Cp || !theta) return -1;
    return eigs_rr::rayleigh_ritz(m, p, MG_EIGS_DROP, G, H, C, Cp, theta);
}

int mg_eigsGram(int N, int m, const double *const *S, const double *const *AS, double *G, double *H)
{
    if (!require_ready("mg_eigsGram")) return MG_ERR_NOT_INIT;
    if (N < 3 || m < 1 || m > k::EIGS_MAX_M || !S || !AS || !G || !H) {
        fail(MG_ERR_ARG, "mg_eigsGram: N = %d < 3, m = %d outside [1, %d], or a NULL array", N, m, k::EIGS_MAX_M);
        return MG_ERR_ARG;
    }
    const hipStream_t st = ctx().stream;
    std::vector<const double *> t(S, S + m);
    t.insert(t.end(), AS, AS + m);
    const size_t n_out = gram_sums(m), n_part = n_out * k::eigs_gram_blocks(N);
    void *block = nullptr;
    if (!MG_HIP(hipMalloc(&block, (2 * (size_t)m) * sizeof(double *) + (n_part + n_out) * sizeof(double)))) return MG_ERR_HIP;
    double *part = static_cast<double *>(block), *out = part + n_part;
    const double **tab = reinterpret_cast<const double **>(out + n_out);
    std::vector<double> host(n_out);
    bool ok = MG_HIP(hipMemcpyAsync(tab, t.data(), t.size() * sizeof(double *), hipMemcpyHostToDevice, st)) && sync(st);
    if (ok) {
        {
            ProfScope ps("eig_gram", N, (double)N * N * 16.0 * m);
            k::eigs_gram(st, N, m, tab, part, out);
        }
        ok = MG_HIP(hipMemcpyAsync(host.data(), out, n_out * sizeof(double), hipMemcpyDeviceToHost, st)) && sync(st);
    }
    (void)hipFree(block);
    if (!ok) return MG_ERR_HIP;
    gram_unpack(m, host.data(), G, H);
    return MG_OK;
}

int mg_eigsRotate(int N, int m, int p, const double *C, const double *Cp, const double *theta, double *const *S, double *const *AS,
                  double *const *R, double *res2)
{
    if (!require_ready("mg_eigsRotate")) return MG_ERR_NOT_INIT;
    if (N < 3 || p < 1 || p > MG_EIGS_MAX_BLOCK || m < p || m > 3 * p || !C || !Cp || !theta || !S || !AS || !R || !res2) {
        fail(MG_ERR_ARG, "mg_eigsRotate: N = %d < 3, p = %d outside [1, %d], m = %d outside [p, 3p], or a NULL array", N, p,
             MG_EIGS_MAX_BLOCK, m);
        return MG_ERR_ARG;
    }
    const hipStream_t st = ctx().stream;
    std::vector<double *> t(k::EIGS_PTR_COUNT, nullptr);
    for (int j = 0; j < 3 * p; ++j) {
        t[j] = S[j];
        t[k::EIGS_PTR_AS + j] = AS[j];
    }
    for (int i = 0; i < p; ++i) t[k::EIGS_PTR_R + i] = R[i];
    std::vector<double> coef(k::EIGS_COEF_COUNT);
    coef_pack(m, p, C, Cp, theta, coef.data());
    const size_t n_part = (size_t)p * k::eigs_rotate_blocks(N);
    void *block = nullptr;
    if (!MG_HIP(hipMalloc(&block, (n_part + MG_EIGS_MAX_BLOCK + k::EIGS_COEF_COUNT) * sizeof(double) + t.size() * sizeof(double *))))
        return MG_ERR_HIP;
    double *part = static_cast<double *>(block), *r2 = part + n_part, *cf = r2 + MG_EIGS_MAX_BLOCK;
    double **tab = reinterpret_cast<double **>(cf + k::EIGS_COEF_COUNT);
    bool ok = MG_HIP(hipMemcpyAsync(tab, t.data(), t.size() * sizeof(double *), hipMemcpyHostToDevice, st)) &&
              MG_HIP(hipMemcpyAsync(cf, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, st)) && sync(st);
    if (ok) {
        {
            ProfScope ps("eig_rotate", N, (double)N * N * (16.0 * m + 40.0 * p));
            k::eigs_rotate(st, N, m, p, tab, cf, part, r2);
        }
        ok = MG_HIP(hipMemcpyAsync(res2, r2, p * sizeof(double), hipMemcpyDeviceToHost, st)) && sync(st);
    }
    (void)hipFree(block);
    return ok ? MG_OK : MG_ERR_HIP;
}

}  // extern "C"
