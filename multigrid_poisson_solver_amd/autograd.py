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
Not differentiated: shift, and anything through HeatStepper."""
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

    def close(self):
        for s in (self._single, self._batch):
            if s is not None:
                s.close()
        self._single = self._batch = None
