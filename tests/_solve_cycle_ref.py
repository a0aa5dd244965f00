"""The launches of one V(pre, post) cycle of the residual-tolerance solvers, restated from the six functions that spelled
the dataflow out before it was recorded once.  Line numbers are those of commit db87170:

    mg_solve.cpp        solve_vcycle :224-272, vcycle_fused :289-338
    mg_solve_batch.cpp  fill_tables :121-153, fill_tables_vc :161-188 (which role of a table entry holds which array),
                        n_tables :74, n_tables_vc :82

A step is (kind, level, steps, d_sign, fused_transfer, in, F, coarse, out, Fc); a field is (FIELD, level), NONE being
(0, 0) and U0 / F0 carrying the cycle's top level.  Written from those functions, not from build_solve_cycle."""
NODE, SWEEP, RESIDUAL, RESTRICT, COARSE, PROLONG_ADD, COPY = range(7)
F_NONE, F_U0, F_F0, F_A, F_B, F_F, F_COEF = range(7)
NONE = (F_NONE, 0)


def ops_cycle(nl, pre, post, top, with_coef):
    """solve_vcycle: operator by operator, cur / other swapping after every sweep and after the prolongation-add."""
    U0, F0 = (F_U0, top), (F_F0, top)
    last = nl - 1
    a = (lambda l: (F_COEF, l)) if with_coef else (lambda l: NONE)   # fill_tables_vc :170, :173-175, :178, :181
    steps, x, y = [], {}, {}
    for l in range(top, last):                                       # :231
        F = F0 if l == top else (F_F, l)                              # :232
        cur, other = (U0 if l == top else (F_A, l)), (F_B, l)         # :233
        sweeps = pre                                                  # :234
        if l > top:                                                   # :235-239 the zero start, folded into the first sweep
            steps.append((SWEEP, l, 0, 0, 0, NONE, F, a(l), cur, NONE))
            sweeps -= 1
        for _ in range(sweeps):                                       # :240-244
            steps.append((SWEEP, l, 0, 0, 0, cur, F, a(l), other, NONE))
            cur, other = other, cur
        steps.append((RESIDUAL, l, 0, 0, 0, cur, F, a(l), other, NONE))            # :246
        steps.append((RESTRICT, l, 0, 0, 0, other, NONE, NONE, (F_F, l + 1), NONE))   # :247
        x[l], y[l] = cur, other                                       # :249-250
    steps.append((COARSE, last, 0, 0, 0, NONE, (F_F, last), a(last), (F_A, last), NONE))   # :252
    x[last] = (F_A, last)                                             # :254
    for l in range(last - 1, top - 1, -1):                            # :255
        F = F0 if l == top else (F_F, l)
        cur, other = x[l], y[l]                                       # :257
        steps.append((PROLONG_ADD, l, 0, 0, 0, cur, NONE, x[l + 1], other, NONE))   # :259
        cur, other = other, cur                                       # :261
        for _ in range(post):                                         # :262-266
            steps.append((SWEEP, l, 0, 0, 0, cur, F, a(l), other, NONE))
            cur, other = other, cur
        x[l] = cur                                                    # :267
    if x[top] != U0:                                                  # :270
        steps.append((COPY, top, 0, 0, 0, x[top], NONE, NONE, U0, NONE))
    return steps


def fused_cycle(nl, pre, post, top, down_fused, up_fused):
    """vcycle_fused: one node per level and direction, the transfers beside it where they do not fuse."""
    U0, F0 = (F_U0, top), (F_F0, top)
    steps, x = [], {}
    for l in range(top, nl - 1):                                      # :295
        F = F0 if l == top else (F_F, l)                              # :299
        inp = U0 if l == top else NONE                                # :300
        out = (F_B, l) if l == top else (F_A, l)                      # :301
        scratch = U0 if l == top else (F_B, l)                        # :301
        if down_fused[l]:                                             # :303-305
            steps.append((NODE, l, pre, -1, 1, inp, F, NONE, out, (F_F, l + 1)))
        else:                                                         # :307-310
            steps.append((NODE, l, pre, -1, 0, inp, F, NONE, out, NONE))
            steps.append((RESIDUAL, l, 0, 0, 0, out, F, NONE, scratch, NONE))
            steps.append((RESTRICT, l, 0, 0, 0, scratch, NONE, NONE, (F_F, l + 1), NONE))
        x[l] = out                                                    # :312
    steps.append((COARSE, nl - 1, 0, 0, 0, NONE, (F_F, nl - 1), NONE, (F_A, nl - 1), NONE))   # :315
    x[nl - 1] = (F_A, nl - 1)                                         # :317
    for l in range(nl - 2, top - 1, -1):                              # :318
        F = F0 if l == top else (F_F, l)                              # :322
        inp, out = x[l], (U0 if l == top else (F_B, l))               # :323
        if up_fused[l]:                                               # :325-328
            steps.append((NODE, l, post, +1, 1, inp, F, x[l + 1], out, NONE))
            x[l] = out
        else:                                                         # :331-334
            steps.append((PROLONG_ADD, l, 0, 0, 0, inp, NONE, x[l + 1], out, NONE))
            steps.append((NODE, l, post, +1, 0, out, F, NONE, inp, NONE))
            x[l] = inp
    if x[top] != U0:                                                  # :337
        steps.append((COPY, top, 0, 0, 0, x[top], NONE, NONE, U0, NONE))
    return steps


def n_tables(nl):      # mg_solve_batch.cpp :74 -- the norm's table, the fused cycle's, the copy's
    return 3 + 5 * (nl - 1)


def n_tables_vc(nl):   # mg_solve_batch.cpp :82
    return 3 + 6 * (nl - 1)
