/*
 * mg_fmg.h -- the two building blocks of the full-multigrid start of the residual-tolerance solver (mg_hip.h:
 * mg_solve_opts.fmg), exported so that a restatement of the pass can be written from the ABI: the host-built interpolation
 * table and the prolongation kernel on its own.  mg_hip.h includes this file; libmgpoisson.so exports both symbols.
 * Memory contract (mg_hip.h): mg_cubic_table takes HOST arrays; mg_prolongCubic reads U_c, writes the interior of U_f and
 * nothing else (tests/test_solve_fmg_gpu.py holds it inside guard bands).
 */
#ifndef MG_FMG_H
#define MG_FMG_H

#ifdef __cplusplus
extern "C" {
#endif

/* 1-D cubic (Lagrange) interpolation from N_src to N_dst equally spaced points over the same interval, the table of the
 * full-multigrid start (mg_solve_opts.fmg).  Destination point i sits at t = i*(N_src-1)/(N_dst-1) in source index units;
 * it reads the m = min(4, N_src) nodes base[i] .. base[i]+m-1, base[i] = clamp(floor(t) - 1, 0, N_src - m), with the
 * Lagrange weights w[4*i + 0..m-1] at t (unused entries 0).  Each weight is formed on the host in long double from the
 * integers i, N_src, N_dst -- one division of two exactly represented integers -- and rounded once to fp64; a node that
 * t coincides with has weight exactly 1, the others exactly +0.  base: N_dst ints, w: 4*N_dst doubles.  N_src, N_dst >= 2. */
void mg_cubic_table(int N_src, int N_dst, int *base, double *w);

/* bicubic interpolation of U_c (N_src x N_src) into the INTERIOR of U_f (N_dst x N_dst; its rim is not written), the
 * prolongation of the full-multigrid start.  With (base, w) = mg_cubic_table(N_src, N_dst) for rows and columns alike, fine
 * point (r, c) is, every product and every sum rounded (no fma), first along the columns of each of the m source rows
 * k = 0..m-1,  v_k = ((w[c][0]*s_k0 + w[c][1]*s_k1) + w[c][2]*s_k2) + w[c][3]*s_k3,  s_kj = U_c[base[r]+k][base[c]+j],
 * then  out = ((w[r][0]*v_0 + w[r][1]*v_1) + w[r][2]*v_2) + w[r][3]*v_3;  for m = 3 (N_src = 3) the last term of both sums
 * is left out.  U_c is read only.  N_src >= 3, N_dst >= 3.  The kernel's tiling holds the source windows of
 * N_src = N_dst/2 (the solver's levels) and of any coarser source; a table it cannot hold is refused with MG_ERR_UNSUPPORTED. */
void mg_prolongCubic(int N_src, const double *U_c, int N_dst, double *U_f);

#ifdef __cplusplus
}
#endif
#endif /* MG_FMG_H */
