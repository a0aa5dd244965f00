"""torch.autograd over the residual-tolerance solvers: a solve  div(a grad U) - sigma*U = F  whose result carries a grad_fn,
with the gradients in F, in the Dirichlet data on the rim of U0 and in the nodal coefficient a coming from ONE adjoint solve
(include/mg_adjoint.h: the discrete operator is symmetric on the interior, so the adjoint equation is the forward equation
with another right-hand side).  The package does not import this module -- torch stays an optional, lazily imported
dependency:

    from multigrid_poisson_solver_amd.autograd import DifferentiableSolver
    ds = DifferentiableSolver(N, L, shift=0.0, rtol=1e-10)
    U = ds.solve(F, U0, a)                    # float64 CUDA tensors (N, N) -- or [B, N, N] with max_batch >= B
    J = 0.5 * ((U - U_obs) ** 2).sum()
    J.backward()                              # F.grad, U0.grad (rim data), a.grad

What the gradients are: the derivatives of the DISCRETE solution as the solver defines it, exact up to the tolerance of the
two solves (forward and adjoint).  dJ/dF is the adjoint field with a zero rim; dJ/dU0 is zero on the interior (the answer does
not depend on the initial guess) and the boundary sensitivity on the rim; dJ/da is given at every grid point, rim included.
Not differentiated: shift, and anything through HeatStepper.

solve_reaction(F, U0, s, a) and solve_semilinear(F, U0, kind, kappa, weight, a) do the same for the equations with a reaction
term s(x, y) and with a semilinear term kappa*w*g(U) (include/mg_adjoint_rx.h), with the gradients in s, in weight and in
kappa beside the three above; the adjoint of the semilinear solve is ONE linear solve at its solution."""
import torch

import multigrid_poisson_solver_amd as mg


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ds, F, U0, a):
        U = U0.detach().clone(memory_format=torch.contiguous_format)
        version = ds._set_coefficient(None if a is None else a.detach())
        infos = ds._forward(F.detach().contiguous(), U)
        ds._require_converged(infos, "forward")
        ds.last_forward_info = infos
        ctx.ds, ctx.version, ctx.has_a = ds, version, a is not None
        ctx.save_for_backward(U, *([a] if a is not None else []))
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, Ubar):
        ds = ctx.ds
        saved = ctx.saved_tensors
        U, a = saved[0], (saved[1] if ctx.has_a else None)
        need_F, need_U0, need_a = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.has_a and ctx.needs_input_grad[3]
        if not (need_F or need_U0 or need_a):
            return None, None, None, None
        if ds._version != ctx.version:   # another forward has replaced the coefficient since: put this one's back
            ctx.version = ds._set_coefficient(None if a is None else a.detach())
        lam, gA, gU, infos = ds._adjoint(Ubar.contiguous(), U, need_a, need_U0)
        ds._require_converged(infos, "adjoint")
        ds.last_adjoint_info = infos
        gF = None
        if need_F:   # lam with its rim set to zero (the solver's prolongation may move a rim value by a rounding)
            gF = lam
            gF[..., 0, :] = 0.0
            gF[..., -1, :] = 0.0
            gF[..., :, 0] = 0.0
            gF[..., :, -1] = 0.0
        if need_a and gA.dim() == 3 and a.dim() == 2:   # one coefficient shared by the instances: the sum over them
            gA = gA.sum(0)
        return None, gF, gU if need_U0 else None, gA if need_a else None


def _zero_rim(lam):
    """lam with its rim set to zero, in place (the solver's prolongation may move a rim value by a rounding)"""
    lam[..., 0, :] = 0.0
    lam[..., -1, :] = 0.0
    lam[..., :, 0] = 0.0
    lam[..., :, -1] = 0.0
    return lam


def _shared_sum(g, x):
    """the gradient in a field x that the instances of a batch share: the sum over them"""
    return g.sum(0) if g.dim() == 3 and x.dim() == 2 else g


class _SolveReaction(torch.autograd.Function):
    """div(a grad U) - (sigma + s)*U = F (include/mg_adjoint_rx.h): the reaction term is set for the length of each solve"""

    @staticmethod
    def forward(ctx, ds, F, U0, s, a):
        U = U0.detach().clone(memory_format=torch.contiguous_format)
        version = ds._set_coefficient(None if a is None else a.detach())
        solver = ds._sync(U.dim() == 3)
        solver.set_reaction(s.detach().contiguous())
        try:
            infos = ds._forward(F.detach().contiguous(), U)
        finally:
            solver.set_reaction(None)
        ds._require_converged(infos, "forward")
        ds.last_forward_info = infos
        ctx.ds, ctx.version, ctx.has_a = ds, version, a is not None
        ctx.save_for_backward(U, s, *([a] if a is not None else []))
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, Ubar):
        ds = ctx.ds
        saved = ctx.saved_tensors
        U, s, a = saved[0], saved[1], (saved[2] if ctx.has_a else None)
        need_F, need_U0, need_s = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        need_a = ctx.has_a and ctx.needs_input_grad[4]
        if not (need_F or need_U0 or need_s or need_a):
            return None, None, None, None, None
        if ds._version != ctx.version:
            ctx.version = ds._set_coefficient(None if a is None else a.detach())
        batched = U.dim() == 3
        solver = ds._sync(batched)
        solver.set_reaction(s.detach().contiguous())
        try:
            lam, gA, gU, gS, info = solver.adjoint_reaction(Ubar.contiguous(), U, want_coef=need_a, want_rim=need_U0, want_reaction=need_s)
        finally:
            solver.set_reaction(None)
        infos = info if batched else [info]
        ds._require_converged(infos, "adjoint")
        ds.last_adjoint_info = infos
        return (None, _zero_rim(lam) if need_F else None, gU if need_U0 else None, _shared_sum(gS, s) if need_s else None,
                _shared_sum(gA, a) if need_a else None)


class _SolveSemilinear(torch.autograd.Function):
    """div(a grad U) - sigma*U - kappa*w*g(U) = F by Newton-multigrid, its adjoint ONE linear solve (include/mg_adjoint_rx.h)"""

    @staticmethod
    def forward(ctx, ds, F, U0, kind, kappa, weight, a, newton_opts):
        U = U0.detach().clone(memory_format=torch.contiguous_format)
        batched = U.dim() == 3
        version = ds._set_coefficient(None if a is None else a.detach())
        solver = ds._sync(batched)
        kap = ds._kappa_values(kappa, U)
        w = None if weight is None else weight.detach().contiguous()
        Fc = F.detach().contiguous()
        if batched:
            infos = list(solver.newton_batch(Fc, U, kind=kind, kappa=kap, weight=w, **newton_opts)[1])
        else:
            infos = [solver.newton(Fc, U, kind=kind, kappa=kap, weight=w, **newton_opts)[1]]
        if ds.strict:
            bad = [i for i, info in enumerate(infos) if not info["converged"]]
            if bad:
                raise mg.MGError(f"DifferentiableSolver: the forward Newton solve of instance(s) {bad} did not converge "
                                 f"(res {infos[bad[0]]['res']:.3e} after {infos[bad[0]]['iterations']} iterations); strict=False returns it anyway")
        ds.last_forward_info = infos
        ctx.ds, ctx.version, ctx.kind, ctx.kap = ds, version, kind, kap
        ctx.has_a, ctx.has_w, ctx.kappa_tensor = a is not None, weight is not None, torch.is_tensor(kappa)
        ctx.save_for_backward(U, Fc, *([weight] if weight is not None else []), *([a] if a is not None else []),
                              *([kappa] if torch.is_tensor(kappa) else []))
        return U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, Ubar):
        ds = ctx.ds
        saved = list(ctx.saved_tensors)
        U, F = saved[0], saved[1]
        rest = saved[2:]
        weight = rest.pop(0) if ctx.has_w else None
        a = rest.pop(0) if ctx.has_a else None
        kappa = rest.pop(0) if ctx.kappa_tensor else None
        need = ctx.needs_input_grad
        need_F, need_U0, need_k, need_w, need_a = need[1], need[2], ctx.kappa_tensor and need[4], ctx.has_w and need[5], ctx.has_a and need[6]
        if not (need_F or need_U0 or need_k or need_w or need_a):
            return (None,) * 8
        if ds._version != ctx.version:
            ctx.version = ds._set_coefficient(None if a is None else a.detach())
        batched = U.dim() == 3
        solver = ds._sync(batched)
        w = None if weight is None else weight.detach().contiguous()
        call = solver.newton_adjoint_batch if batched else solver.newton_adjoint
        lam, gA, gU, gW, info = call(Ubar.contiguous(), U, F, kind=ctx.kind, kappa=ctx.kap, weight=w, want_coef=need_a, want_rim=need_U0,
                                     want_weight=need_w or need_k)
        infos = info if batched else [info]
        ds._require_converged(infos, "adjoint")
        ds.last_adjoint_info = infos
        gk = None
        if need_k:   # one value per instance; a 0-dim kappa is shared by the instances: the sum over them
            vals = torch.tensor([i["gkappa"] for i in infos], dtype=torch.float64, device=kappa.device)
            gk = vals.sum() if kappa.dim() == 0 and batched else vals.reshape(kappa.shape)
        return (None, _zero_rim(lam) if need_F else None, gU if need_U0 else None, None, gk,
                _shared_sum(gW, weight) if need_w else None, _shared_sum(gA, a) if need_a else None, None)


class DifferentiableSolver:
    """A Solver (inputs of shape (N, N)) and, for inputs of shape [B, N, N], a BatchSolver for up to max_batch instances,
    whose solve() is differentiable.  **opts are the solve options of solve_opts (shift, rtol, pre, post, ...) plus krylov=m.
    strict=True: a forward or adjoint solve that does not converge raises MGError instead of returning a gradient of
    unknown quality.  Solves run in place on torch.cuda.current_stream()."""

    def __init__(self, N, L=1.0, max_batch=1, strict=True, **opts):
        self.N, self.L, self.max_batch, self.strict = int(N), float(L), int(max_batch), bool(strict)
        self._krylov = int(opts.pop("krylov", 0))
        self._opts = dict(opts)
        self._single = self._batch = None
        self._version = 0          # counts set_coefficient calls: a backward re-sets its own coefficient when it is stale
        self._coef = None          # the coefficient the solvers hold now (a detached tensor, or None)
        self.last_forward_info = self.last_adjoint_info = None

    # ---------------------------------------------------------------- the solvers
    def _solver(self, batched):
        if batched:
            if self._batch is None:
                self._batch = mg.BatchSolver(self.N, self.L, max_batch=self.max_batch, **self._opts)
                if self._krylov:
                    self._batch.set_krylov(self._krylov)
                self._batch_version = -1
            return self._batch
        if self._single is None:
            self._single = mg.Solver(self.N, self.L, krylov=self._krylov, **self._opts)
            self._single_version = -1
        return self._single

    def _set_coefficient(self, a):
        """note the coefficient of the coming solves; the solver that runs them takes it over lazily (_sync)"""
        self._version += 1
        self._coef = a
        return self._version

    def _sync(self, batched):
        s = self._solver(batched)
        attr = "_batch_version" if batched else "_single_version"
        if getattr(self, attr) != self._version:
            a = self._coef
            if a is None:
                if s.has_coefficient:
                    s.set_coefficient(None)
            else:
                s.set_coefficient(a if a.is_contiguous() else a.contiguous())
            setattr(self, attr, self._version)
        return s

    def _forward(self, F, U):
        batched = U.dim() == 3
        s = self._sync(batched)
        if batched:
            return s.solve(F, U)[1]
        return [s.solve(F, U)[1]]

    def _adjoint(self, Ubar, U, want_coef, want_rim):
        batched = U.dim() == 3
        s = self._sync(batched)
        lam, gA, gU, info = s.adjoint(Ubar, U, want_coef=want_coef, want_rim=want_rim)
        return lam, gA, gU, info if batched else [info]

    def _require_converged(self, infos, what):
        if self.strict:
            bad = [i for i, info in enumerate(infos) if not info["converged"]]
            if bad:
                raise mg.MGError(f"DifferentiableSolver: the {what} solve of instance(s) {bad} did not converge "
                                 f"(res {infos[bad[0]]['res']:.3e} after {infos[bad[0]]['cycles']} cycles); strict=False returns it anyway")

    # ---------------------------------------------------------------- the interface
    def solve(self, F, U0, a=None):
        """U with a grad_fn: the solution of div(a grad U) - sigma*U = F with the rim of U0 as Dirichlet data and its interior
        as the initial guess (U0 is cloned, not written).  F, U0: float64 CUDA tensors of shape (N, N) or [B, N, N],
        B <= max_batch; a: None (a = 1), (N, N) -- for a batch: shared by the instances -- or [B, N, N]."""
        N = self.N
        for name, t in (("F", F), ("U0", U0)) + ((("a", a),) if a is not None else ()):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape[-2:]) == (N, N) and t.dim() in (2, 3)):
                raise mg.MGError(f"{name}: expected a float64 CUDA tensor of shape ({N}, {N}) or [B, {N}, {N}]")
        if F.shape != U0.shape:
            raise mg.MGError(f"F of shape {tuple(F.shape)} for U0 of shape {tuple(U0.shape)}")
        if U0.dim() == 3 and U0.shape[0] > self.max_batch:
            raise mg.MGError(f"{U0.shape[0]} instances for max_batch = {self.max_batch}")
        if a is not None and a.dim() == 3 and (U0.dim() != 3 or a.shape[0] != U0.shape[0]):
            raise mg.MGError(f"a of shape {tuple(a.shape)} for U0 of shape {tuple(U0.shape)}")
        return _Solve.apply(self, F, U0, a)

    def _check_fields(self, F, U0, optional):
        """F and U0 as solve() takes them; optional: (name, tensor or None) pairs of fields of shape (N, N) -- for a batch: shared
        by the instances -- or [B, N, N]"""
        N = self.N
        for name, t in (("F", F), ("U0", U0)) + tuple((n, t) for n, t in optional if t is not None):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape[-2:]) == (N, N) and t.dim() in (2, 3)):
                raise mg.MGError(f"{name}: expected a float64 CUDA tensor of shape ({N}, {N}) or [B, {N}, {N}]")
        if F.shape != U0.shape:
            raise mg.MGError(f"F of shape {tuple(F.shape)} for U0 of shape {tuple(U0.shape)}")
        if U0.dim() == 3 and U0.shape[0] > self.max_batch:
            raise mg.MGError(f"{U0.shape[0]} instances for max_batch = {self.max_batch}")
        for name, t in optional:
            if t is not None and t.dim() == 3 and (U0.dim() != 3 or t.shape[0] != U0.shape[0]):
                raise mg.MGError(f"{name} of shape {tuple(t.shape)} for U0 of shape {tuple(U0.shape)}")

    def _kappa_values(self, kappa, U):
        """kappa as the solvers take it: a float for one problem, a list of B floats for a batch"""
        B = U.shape[0] if U.dim() == 3 else None
        if torch.is_tensor(kappa):
            if kappa.dtype != torch.float64 or kappa.dim() > 1 or (kappa.dim() == 1 and (B is None or kappa.shape[0] != B)):
                raise mg.MGError(f"kappa: expected a float, or a 0-dim or ({B},) float64 tensor, got shape {tuple(kappa.shape)}")
            vals = kappa.detach().cpu().reshape(-1).tolist()
        else:
            vals = [float(kappa)]
        if B is None:
            return vals[0]
        return vals * B if len(vals) == 1 else vals

    def solve_reaction(self, F, U0, s, a=None):
        """U with a grad_fn: the solution of div(a grad U) - (sigma + s)*U = F (include/mg_adjoint_rx.h), F, U0 and a as solve()
        takes them, s >= 0 of shape (N, N) -- for a batch: shared by the instances -- or [B, N, N].  backward() gives the
        gradients in F, in the rim of U0, in a and in s from ONE adjoint solve; a shared a or s receives the sum over the
        instances.  The reaction term is set for the length of each solve: the solvers have none afterwards."""
        self._check_fields(F, U0, (("s", s), ("a", a)))
        if s is None:
            raise mg.MGError("s: expected a float64 CUDA tensor (solve() is the solve without a reaction term)")
        return _SolveReaction.apply(self, F, U0, s, a)

    def solve_semilinear(self, F, U0, kind="sinh", kappa=1.0, weight=None, a=None, **newton_opts):
        """U with a grad_fn: the solution of div(a grad U) - sigma*U - kappa*w*g(U) = F by Newton-multigrid (Solver.newton,
        BatchSolver.newton_batch; include/mg_adjoint_rx.h), g = u^3 ("cubic"), sinh u ("sinh") or e^u ("exp").  F, U0 and a as
        solve() takes them; weight = w >= 0: None (w = 1), (N, N) -- for a batch: shared -- or [B, N, N]; kappa: a float, or a
        0-dim or (B,) float64 tensor, which may require grad; **newton_opts: rtol, atol, max_iters, max_backtracks of the Newton
        iteration.  backward() gives the gradients in F, in the rim of U0, in a, in weight and in kappa from ONE linear adjoint
        solve at the solution; a shared a, weight or kappa receives the sum over the instances.  strict=True raises on a
        forward Newton solve or an adjoint solve that did not converge."""
        self._check_fields(F, U0, (("weight", weight), ("a", a)))
        return _SolveSemilinear.apply(self, F, U0, kind, kappa, weight, a, dict(newton_opts))

    def close(self):
        for s in (self._single, self._batch):
            if s is not None:
                s.close()
        self._single = self._batch = None
