// mg_eigs_rr.h -- the host side of the eigen-solver's Rayleigh-Ritz step (include/mg_eigs.h): a cyclic Jacobi eigen-solver
// for small symmetric matrices and the step itself.  Plain C++ with no dependency on HIP or on the rest of the engine, so
// that a stand-alone program can compile this very file (tests/test_eigs_cpu.py does, also under a sanitizer).
// Deterministic: fixed sweep order, no threads, no library call beyond sqrt and fabs.
#ifndef MG_EIGS_RR_H
#define MG_EIGS_RR_H

#include <cmath>
#include <cstddef>
#include <vector>

namespace mg {
namespace eigs_rr {

// Eigen-decomposition of the symmetric n x n matrix A (row-major; only its upper triangle is read): w ascending, the
// eigenvector of w[i] in column i of V (row-major, V[r*n + i]).  Cyclic Jacobi, rows p < q in order, until a whole sweep
// rotates nothing (an off-diagonal entry below 2^-60 of sqrt|a_pp*a_qq| -- or an exact zero -- is set to zero instead).
// Ties in w keep the order of the diagonal they came from.  Returns the sweeps taken, -1 when 64 did not suffice.
inline int jacobi_eig(int n, const double *A, double *w, double *V)
{
    std::vector<double> a((size_t)n * n);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) a[(size_t)r * n + c] = r <= c ? A[(size_t)r * n + c] : A[(size_t)c * n + r];
    std::vector<double> v((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    const double tiny = std::ldexp(1.0, -60);
    int sweeps = 0;
    bool rotated = n > 1;
    while (rotated && sweeps < 64) {
        rotated = false;
        ++sweeps;
        for (int p = 0; p + 1 < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
                if (std::fabs(apq) <= tiny * std::sqrt(std::fabs(app * aqq))) {
                    a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
                    continue;
                }
                rotated = true;
                const double zeta = (aqq - app) / (2.0 * apq);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < n; ++k) {   // columns p and q of a
                    const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
                    a[(size_t)k * n + p] = c * akp - s * akq;
                    a[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {   // rows p and q of a
                    const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
                    a[(size_t)p * n + k] = c * apk - s * aqk;
                    a[(size_t)q * n + k] = s * apk + c * aqk;
                }
                a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - s * vkq;
                    v[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i) {   // stable insertion sort by the diagonal
        const int o = order[i];
        int j = i;
        while (j > 0 && a[(size_t)order[j - 1] * n + order[j - 1]] > a[(size_t)o * n + o]) {
            order[j] = order[j - 1];
            --j;
        }
        order[j] = o;
    }
    for (int i = 0; i < n; ++i) {
        w[i] = a[(size_t)order[i] * n + order[i]];
        for (int r = 0; r < n; ++r) V[(size_t)r * n + i] = v[(size_t)r * n + order[i]];
    }
    return rotated ? -1 : sweeps;
}

// The Rayleigh-Ritz step of include/mg_eigs.h on G, H (m x m row-major, upper triangles read): C, Cp (m x p row-major) and
// theta (p).  Returns the directions kept; below p (the breakdown; 0 for a G_jj that is not finite and > 0, and for a G or H on which
// the Jacobi sweeps do not end or that gives a theta that is not finite) nothing is written.
inline int rayleigh_ritz(int m, int p, double drop, const double *G, const double *H, double *C, double *Cp, double *theta)
{
    std::vector<double> d(m), Gh((size_t)m * m), Hh((size_t)m * m);
    for (int j = 0; j < m; ++j) {
        const double g = G[(size_t)j * m + j];
        if (!(g > 0.0) || !(g < HUGE_VAL)) return 0;
        d[j] = 1.0 / std::sqrt(g);
    }
    for (int j = 0; j < m; ++j)
        for (int l = j; l < m; ++l) {
            Gh[(size_t)j * m + l] = Gh[(size_t)l * m + j] = d[j] * G[(size_t)j * m + l] * d[l];
            Hh[(size_t)j * m + l] = Hh[(size_t)l * m + j] = d[j] * H[(size_t)j * m + l] * d[l];
        }
    std::vector<double> w(m), V((size_t)m * m);
    if (jacobi_eig(m, Gh.data(), w.data(), V.data()) < 0) return 0;   // (a matrix that is not finite: the breakdown)
    const double wmax = w[m - 1];
    std::vector<int> keep;
    for (int j = 0; j < m; ++j)
        if (w[j] > drop * wmax) keep.push_back(j);
    const int nk = (int)keep.size();
    if (nk < p) return nk;
    std::vector<double> T((size_t)m * nk), HT((size_t)m * nk), A2((size_t)nk * nk);
    for (int c = 0; c < nk; ++c) {
        const double s = 1.0 / std::sqrt(w[keep[c]]);
        for (int r = 0; r < m; ++r) T[(size_t)r * nk + c] = V[(size_t)r * m + keep[c]] * s;
    }
    for (int r = 0; r < m; ++r)
        for (int c = 0; c < nk; ++c) {
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc += Hh[(size_t)r * m + j] * T[(size_t)j * nk + c];
            HT[(size_t)r * nk + c] = acc;
        }
    for (int r = 0; r < nk; ++r)
        for (int c = r; c < nk; ++c) {   // (the upper triangle is what jacobi_eig reads)
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc += T[(size_t)j * nk + r] * HT[(size_t)j * nk + c];
            A2[(size_t)r * nk + c] = A2[(size_t)c * nk + r] = acc;
        }
    std::vector<double> th(nk), Y((size_t)nk * nk);
    if (jacobi_eig(nk, A2.data(), th.data(), Y.data()) < 0) return 0;
    for (int i = 0; i < p; ++i)
        if (!(th[i] > -HUGE_VAL && th[i] < HUGE_VAL)) return 0;
    for (int i = 0; i < p; ++i) theta[i] = th[i];
    for (int r = 0; r < m; ++r)
        for (int i = 0; i < p; ++i) {
            double acc = 0.0;
            for (int c = 0; c < nk; ++c) acc += T[(size_t)r * nk + c] * Y[(size_t)c * nk + i];
            C[(size_t)r * p + i] = d[r] * acc;
            Cp[(size_t)r * p + i] = r < p ? 0.0 : d[r] * acc;
        }
    return nk;
}

// The same step on the basis columns with active[j] != 0 only (the first p columns, X, must be active): the rows of C and Cp
// of the others are +0.  Returns the directions kept.
inline int rayleigh_ritz_masked(int m, int p, double drop, const char *active, const double *G, const double *H, double *C,
                                double *Cp, double *theta)
{
    std::vector<int> idx;
    for (int j = 0; j < m; ++j)
        if (active[j]) idx.push_back(j);
    const int ma = (int)idx.size();
    if (ma == m) return rayleigh_ritz(m, p, drop, G, H, C, Cp, theta);
    if (ma < p) return ma;
    std::vector<double> Ga((size_t)ma * ma), Ha((size_t)ma * ma), Ca((size_t)ma * p), Cpa((size_t)ma * p);
    for (int r = 0; r < ma; ++r)
        for (int c = 0; c < ma; ++c) {
            Ga[(size_t)r * ma + c] = G[(size_t)idx[r] * m + idx[c]];
            Ha[(size_t)r * ma + c] = H[(size_t)idx[r] * m + idx[c]];
        }
    const int kept = rayleigh_ritz(ma, p, drop, Ga.data(), Ha.data(), Ca.data(), Cpa.data(), theta);
    if (kept < p) return kept;
    for (size_t i = 0; i < (size_t)m * p; ++i) C[i] = Cp[i] = 0.0;
    for (int r = 0; r < ma; ++r)
        for (int i = 0; i < p; ++i) {
            C[(size_t)idx[r] * p + i] = Ca[(size_t)r * p + i];
            Cp[(size_t)idx[r] * p + i] = Cpa[(size_t)r * p + i];
        }
    return kept;
}

}  // namespace eigs_rr
}  // namespace mg

#endif /* MG_EIGS_RR_H */
