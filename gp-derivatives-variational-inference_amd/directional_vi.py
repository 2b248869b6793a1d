"""DSVGP training / evaluation harness -- drop-in mirror of the reference
``directionalvi/directional_vi.py`` (``GPModel`` :25-65, ``select_cols_of_y`` :68-90, ``train_gp`` :93-268,
``eval_gp`` :271-305): same names, arguments, defaults, return types and interleaved output ordering.

What is different underneath (MI355X-first):
  * the dataset is made resident in HBM once; each step's minibatch is gathered on the GPU
    (``dsvgp_gather_batch`` / ``dsvgp_gather_batch_f64``) from a per-epoch ``randperm`` instead of ``DataLoader``'s per-index collate
    plus a host->device copy per step (directional_vi.py:133,229-232);
  * ``likelihood(model(x))`` + ``mll`` + ``backward`` run as one fused HIP forward/backward (``_step.py``);
  * both Adam optimizers are the fused HIP Adam (``optim.FusedAdam``), stepped with the same
    per-iteration LR schedulers as the reference (:251-254);
  * under ``torch.distributed`` (one process per GPU) every global minibatch is sharded by rows and
    gradients are reduced with one RCCL all-reduce (``parallel.DataParallel``).
``use_ngd=True`` swaps q(u) for a NaturalVariationalDistribution stepped by ``optim.NGD`` (reference :35-37,186-187) on the
same engine; ``use_ciq=True`` additionally whitens with K_ZZ^{-1/2} by contour-integral quadrature + msMINRES
(``CiqDirectionalGradVariationalStrategy``, ``csrc/ciq.hip``).
"""
import collections
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

from . import _ops
from .CiqDirectionalGradVariationalStrategy import CiqDirectionalGradVariationalStrategy
from .DirectionalGradVariationalStrategy import DirectionalGradVariationalStrategy
from .Matern52KernelDirectionalGrad import Matern52KernelDirectionalGrad
from .RBFKernelDirectionalGrad import RBFKernelDirectionalGrad
from .gp_shim import (ApproximateGP, CholeskyVariationalDistribution, ConstantMean, GaussianLikelihood,
                      NaturalVariationalDistribution, PredictiveLogLikelihood, ScaleKernel, VariationalELBO)
from . import optim as _optim
from .optim import NGD, FusedAdam, make_adam
from .parallel import DataParallel


class GPModel(ApproximateGP):
    def __init__(self, inducing_points, inducing_directions, dim, learn_inducing_locations=True, ard_num_dims=None, **kwargs):
        # ``ard_num_dims`` (int, not in the reference; None = one scalar lengthscale): one lengthscale per input dimension,
        # raw_lengthscale [1, ard_num_dims] under the same state_dict key, as gpytorch's RBFKernel(ard_num_dims=)
        # ``kernel`` (through **kwargs, like ``variational_strategy``; "rbf" by default): "matern52" builds the model on
        # Matern52KernelDirectionalGrad -- gpytorch's MaternKernel(nu=2.5, ard_num_dims=) -- with the same parameters under the same keys
        torch.nn.Module.__init__(self)
        self.num_inducing = len(inducing_points)
        self.num_directions = int(len(inducing_directions) / self.num_inducing)  # num directions per point
        num_directional_derivs = self.num_directions * self.num_inducing
        if kwargs.get("variational_distribution") == "NGD":                       # :35-37
            variational_distribution = NaturalVariationalDistribution(self.num_inducing + num_directional_derivs)
        else:
            variational_distribution = CholeskyVariationalDistribution(self.num_inducing + num_directional_derivs)
        self._ciq = kwargs.get("variational_strategy") == "CIQ"
        if self._ciq:                                                             # :46-48
            variational_strategy = CiqDirectionalGradVariationalStrategy(
                self, inducing_points, inducing_directions, variational_distribution,
                learn_inducing_locations=learn_inducing_locations)
        else:
            strategy_class = getattr(self, "_strategy_class", None) or DirectionalGradVariationalStrategy
            variational_strategy = strategy_class(
                self, inducing_points, inducing_directions, variational_distribution,
                learn_inducing_locations=learn_inducing_locations)
        self.variational_strategy = variational_strategy
        self._engine = None
        self.data_parallel = None
        self.data_directions = None             # int: the data carry that many directions per point, not num_directions (ApproximateGP)
        # ``missing_targets`` (through **kwargs; False by default): NaN targets are observations that do not exist -- the engine's masked
        # per-output step and collapsed statistics (``ElboEngine.missing_targets``)
        self.missing_targets = bool(kwargs.get("missing_targets", False))
        self.mean_module = ConstantMean()
        if ard_num_dims is not None and int(ard_num_dims) != int(dim):
            raise ValueError("ard_num_dims must equal the input dimension (%d), got %s" % (dim, ard_num_dims))
        kernel = kwargs.get("kernel", "rbf")
        if kernel not in ("rbf", "matern52"):
            raise ValueError("kernel must be 'rbf' or 'matern52', got %r" % (kernel,))
        if kernel == "matern52" and (self._ciq or kwargs.get("variational_distribution") == "NGD"):
            raise ValueError("the Matern-5/2 kernel is built for the Cholesky-whitened model (not CIQ / natural parameters)")
        kernel_class = Matern52KernelDirectionalGrad if kernel == "matern52" else RBFKernelDirectionalGrad
        self.covar_module = ScaleKernel(kernel_class(ard_num_dims=ard_num_dims))
        if self._ciq:
            # stable initialization of lengthscale for CIQ (:58-60): lengthscale = 1 / num_inducing through the
            # inverse of the softplus constraint
            ell = torch.tensor(1.0 / self.num_inducing)
            with torch.no_grad():
                self.covar_module.base_kernel.raw_lengthscale.fill_(float(torch.log(torch.expm1(ell))))

    @property
    def engine(self):
        eng = ApproximateGP.engine.fget(self)
        eng.whitening = "ciq" if self._ciq else "cholesky"
        eng.data_outputs = "all"
        eng.shared_directions = False
        eng.kernel = "matern52" if isinstance(self.covar_module.base_kernel, Matern52KernelDirectionalGrad) else "rbf"
        eng.missing_targets = bool(getattr(self, "missing_targets", False))
        return eng

    # --- parameter plumbing for the HIP engine (order = _step.PARAM_NAMES) ---
    def _param_list(self, likelihood=None):
        vs = self.variational_strategy
        vd = vs._variational_distribution
        raw_noise = (likelihood.noise_covar.raw_noise if likelihood is not None
                     else torch.zeros(1, device=vs.inducing_points.device))
        q = ([vd.natural_vec, vd.natural_mat] if isinstance(vd, NaturalVariationalDistribution)
             else [vd.variational_mean, vd.chol_variational_covar])
        return [vs.inducing_points, vs.inducing_directions] + q + [
            self.mean_module.constant, self.covar_module.raw_outputscale,
            self.covar_module.base_kernel.raw_lengthscale, raw_noise] + (
                [likelihood.noise_covar.raw_derivative_noise] if getattr(likelihood, "has_derivative_noise", False) else [])

    def _param_names(self, likelihood=None):
        from ._step import DERIVATIVE_NOISE, NGD_PARAM_NAMES, PARAM_NAMES
        ngd = isinstance(self.variational_strategy._variational_distribution, NaturalVariationalDistribution)
        names = NGD_PARAM_NAMES if ngd else PARAM_NAMES
        # (a likelihood with a second noise: its parameter rides behind the fixed names -- the engine's switch is its presence)
        return names + (DERIVATIVE_NOISE,) if getattr(likelihood, "has_derivative_noise", False) else names

    def _param_dict(self, likelihood=None):
        return {k: _ops.detach_keep(v) for k, v in zip(self._param_names(likelihood), self._param_list(likelihood))}


def select_cols_of_y(y_batch, minibatch_dim, dim):
    """
    randomly select columns of y to train on, but always select function values as part of the batch
    (reference directional_vi.py:68-90).  Returns (y_batch[:, idx], canonical derivative directions).
    """
    idx_y = random.sample(range(1, dim + 1), minibatch_dim)  # ensures unique entries
    idx_y += [0]  # append 0 to the list for function values
    idx_y.sort()
    y_batch = y_batch[:, idx_y]
    E_canonical = torch.eye(dim).to(y_batch.device)
    derivative_directions = E_canonical[np.array(idx_y[1:]) - 1]
    return y_batch, derivative_directions


def _dataset_tensors(dataset, device, dtype=None):
    """Materialise a torch Dataset of (x[d], y[d+1]) pairs as two HBM-resident matrices: float32, or float64 when the
    process runs with ``torch.set_default_dtype(torch.float64)`` like the reference's experiment scripts (exp_script.py:56)."""
    if dtype is None:
        dtype = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
    tensors = getattr(dataset, "tensors", None)
    if tensors is not None and len(tensors) == 2:
        X, Y = tensors
    else:
        xs, ys = zip(*[dataset[i] for i in range(len(dataset))])
        X, Y = torch.stack(xs), torch.stack(ys)
    return (X.to(device=device, dtype=dtype).contiguous(),
            Y.to(device=device, dtype=dtype).contiguous())


class TrainLoop:
    """State of one training run: resident dataset, model, the two optimizers / schedulers and the
    per-iteration body of the reference loop (directional_vi.py:229-254).  ``train_gp`` drives it over
    shuffled epochs; ``bench.py`` drives the same ``step`` for its timed region."""

    def __init__(self, X, Y, model, likelihood, mll, optimizers, schedulers, minibatch_dim, dp, col_rng, perm_gen,
                 full_gradient=False, dfree=False):
        self.X, self.Y, self.model, self.likelihood, self.mll = X, Y, model, likelihood, mll
        self.variational_optimizer, self.hyperparameter_optimizer = optimizers
        self.variational_scheduler, self.hyperparameter_scheduler = schedulers
        self.minibatch_dim, self.dp, self.col_rng, self.perm_gen = minibatch_dim, dp, col_rng, perm_gen
        self.autograd_protocol = False          # True: loss = -mll(output, y); loss.backward() through torch.autograd
        self.full_gradient = full_gradient      # grad_svgp: all d+1 target columns, no derivative_directions kwarg
        self.dfree = dfree                      # dfree_directional_vi: function values only, first p canonical directions
        self.device = X.device
        self.dim = X.shape[1]
        self.ctx = _ops.Context.get(self.device)
        self.E_canonical = torch.eye(self.dim, device=self.device, dtype=X.dtype)
        self.graph = None                       # HIP-graph replay of the step: True = on (also DSVGP_GRAPH=1), None / False = eager
        self._graphs, self._graph_seen, self._graph_pending = {}, {}, None
        self._deferred_pending = None       # (idx, idx_y, learning rates) of an eager step whose factorisation status has not been read yet
        self.defer_status = None            # None: DSVGP_DEFER_STATUS (default off); True / False
        # int: every minibatch carries that many derivative columns (canonical directions) per point instead of the model's
        # ``minibatch_dim`` -- the rectangular training step of the engine (eager piecewise path: no graph replay, no deferred status)
        self.data_directions = None

    def epoch_permutation(self):
        return torch.randperm(self.X.shape[0], device=self.device, generator=self.perm_gen)   # DataLoader(shuffle=True)

    def step(self, idx, need_variance=False):
        """One optimisation step on the GLOBAL minibatch ``idx`` (row indices into the dataset).
        ``need_variance``: True = the caller will read ``output.variance`` of THIS forward, so the per-output path is used
        instead of the ELBO fast path; "values" = only the function-value rows are read (the reference's every-50-steps nll
        print, :255-260: ``output.variance.sqrt()[::num_directions + 1]``) -- the step stays on the fast path and
        ``output.value_variance`` is formed from the A it leaves behind, before the optimizers change the parameters."""
        eng = self.model.engine
        self._values_only = False
        if need_variance == "values":
            ok = (hasattr(eng, "value_variances") and self.mll.mll_type == "ELBO" and eng.whitening == "cholesky"
                  and not eng.shared_directions and not self.dfree and not getattr(self, "plain", False)
                  and hasattr(self.model.variational_strategy._variational_distribution, "chol_variational_covar")
                  and not self.autograd_protocol)
            self._values_only, need_variance = ok, not ok
        eng.elbo_fast = not need_variance
        dim, p, dp = self.dim, self.minibatch_dim, self.dp
        if self.data_directions is not None:
            p = self.data_directions                    # columns drawn per minibatch (their directions: the matching rows of E_canonical)
        if dp is not None:
            dp.global_batch = idx.shape[0]
            dp.replicated_step = idx.shape[0] < dp.world      # tail smaller than the world: no empty shards (see parallel.py)
            if not dp.replicated_step:
                lo, hi = dp.shard_bounds(idx.shape[0])
                idx = idx[lo:hi]
        # select random columns of y to train on (function values always included), :68-90
        if self.dfree or getattr(self, "plain", False):      # scalar targets: dfree_directional_vi / traditional_vi
            idx_y = [0]
        else:
            idx_y = list(range(dim + 1)) if self.full_gradient else sorted(self.col_rng.sample(range(1, dim + 1), p) + [0])
        if self._graph_eligible(need_variance):
            self._deferred_check_previous()
            return self._graph_step(idx, idx_y)
        if self._graph_pending is not None:
            self._graph_check_previous()
        self._deferred_check_previous()
        return self._eager_step(idx, idx_y, defer=self._defer_eligible(need_variance))

    # ---- deferred status of the one-call step (round 6) -------------------------------------------------------------------------------
    # The eager loop waited ~100 us per step at M' = 600 for the factorisation's status before it queued the optimizers' update.  Now the
    # update is queued at once, guarded ON THE DEVICE by the status word (optim.step_together(guard=)), and the status of step t is read before
    # step t + 1 is queued -- by then it has long arrived.  A failed factorisation (parameters untouched) is redone eagerly through
    # psd_safe_cholesky's jitter ladder, exactly as the graph replay does it (_graph_check_previous).  OPT-IN (``loop.defer_status = True`` /
    # DSVGP_DEFER_STATUS=1): measured at C2 / C3 / C4 on one box, alternating, the step time does not move (0.505-0.528 against 0.505-0.511 /
    # 6.28-6.30 / 11.96-12.01 against 11.95-11.98 ms: the device, not the host, bounds those steps) -- it takes the host's jitter out of the
    # small-problem step, nothing more.
    def _defer_eligible(self, need_variance):
        mode = getattr(self, "defer_status", None)
        if mode is None:
            mode = os.environ.get("DSVGP_DEFER_STATUS", "0") == "1"
        if not mode or need_variance or self.dp is not None or self.autograd_protocol or self.data_directions is not None:
            return False
        eng = self.model.engine
        # (deferral is a float32 feature and stays off under ``deterministic``.  A float64 model never defers -- last clause -- and its loop
        # keeps the one-call step under ``deterministic``: ElboEngine64._c_step64_eligible does not look at the flag, dsvgp_elbo_step_f64
        # itself runs on one stream with fixed-order sums then.)
        return (eng.whitening == "cholesky" and not eng.shared_directions and self.mll.mll_type == "ELBO" and eng.collective is None
                and getattr(eng, "c_step", True) and not getattr(eng, "deterministic", False) and not getattr(eng, "host_trace", None)
                and _optim.can_step_together([self.variational_optimizer, self.hyperparameter_optimizer])
                and self.X.dtype == torch.float32)

    def _deferred_check_previous(self):
        pend, self._deferred_pending = getattr(self, "_deferred_pending", None), None
        if pend is None:
            return
        if self.model.engine.deferred_check() == 0:
            return
        # K_ZZ + 1e-3 I was not positive definite in fp64: the guarded update did nothing; redo the step with the learning rates and step
        # counts it was issued with (jitter ladder of psd_safe_cholesky, NotPSDError after three tries)
        idx, idx_y, lrs_then = pend
        opts = (self.variational_optimizer, self.hyperparameter_optimizer)
        lrs_now = [[g["lr"] for g in o.param_groups] for o in opts]
        for o, ls in zip(opts, lrs_then):
            for g, lr in zip(o.param_groups, ls):
                g["lr"] = lr
                for prm in g["params"]:
                    if o.state.get(prm):
                        o.state[prm]["step"] -= 1
        try:
            cols = torch.tensor(idx_y, dtype=torch.int32, device=self.device)
            self._device_step(idx.contiguous(), cols, len(idx_y) - 1)
            if not _optim.step_together(list(opts)):
                for o in opts:
                    o.step()
        finally:
            for o, ls in zip(opts, lrs_now):
                for g, lr in zip(o.param_groups, ls):
                    g["lr"] = lr

    def _eager_step(self, idx, idx_y, defer=False):
        dp = self.dp
        eng = self.model.engine
        eng.defer_status = bool(defer)
        # host -> device without a stream sync: pinned staging ring + non_blocking copy (a pageable torch.tensor(...,
        # device=) blocks the host until the stream has drained, i.e. until the previous step has finished)
        slot = self._cols_slot = (getattr(self, "_cols_slot", -1) + 1) % 8
        if not hasattr(self, "_cols_pinned") or self._cols_pinned.shape[1] != len(idx_y):
            self._cols_pinned = torch.empty(8, len(idx_y), dtype=torch.int32).pin_memory()
        self._cols_pinned[slot].copy_(torch.tensor(idx_y, dtype=torch.int32))
        cols = self._cols_pinned[slot].to(self.device, non_blocking=True)
        loss, output, y_batch = self._device_step(idx.contiguous(), cols, len(idx_y) - 1)
        output._value_stride = len(idx_y)
        if self._values_only and getattr(self.model.engine, "_last_fast", None) is not None:
            output._value_varn = self.model.engine.value_variances(self.model._param_dict(self.likelihood))
        eng.defer_status = False
        guard = eng.deferred_guard() if defer else None          # (None: the step took a path that read its status itself)
        if guard is not None:
            lrs = [[g["lr"] for g in o.param_groups] for o in (self.variational_optimizer, self.hyperparameter_optimizer)]
            ok = _optim.step_together([self.variational_optimizer, self.hyperparameter_optimizer], guard=guard)
            assert ok                                            # (_defer_eligible: both are FusedAdam; hooks would have made it False)
            self._deferred_pending = (idx, list(idx_y), lrs)
            self.variational_scheduler.step()
            self.hyperparameter_scheduler.step()
        elif _optim.step_together([self.variational_optimizer, self.hyperparameter_optimizer]):      # both Adam: one multi-tensor launch
            self.variational_scheduler.step()
            self.hyperparameter_scheduler.step()
        else:
            self.variational_optimizer.step()
            self.variational_scheduler.step()
            self.hyperparameter_optimizer.step()
            self.hyperparameter_scheduler.step()
        if dp is not None and dp.check_every > 0:
            self._check_replicas(dp)
        return loss, output, y_batch

    def _check_replicas(self, dp, force=False):
        """DSVGP_DP_CHECK (parallel.DataParallel.check_replicas): every N-th step the replicas compare the parameters nobody reduces
        after the update -- all of them: an Adam step on identical gradients keeps identical replicas identical -- and on a mismatch
        take rank 0's parameters AND rank 0's Adam moments (a replica that drifted once would otherwise drift again)."""
        params = [q for opt in (self.variational_optimizer, self.hyperparameter_optimizer)
                  for g in opt.param_groups for q in g["params"]]
        same = dp.check_replicas([q.data for q in params], force=force)
        if not same:
            import torch.distributed as dist
            for opt in (self.variational_optimizer, self.hyperparameter_optimizer):
                for g in opt.param_groups:
                    for q in g["params"]:
                        st = opt.state.get(q)
                        for k in ("exp_avg", "exp_avg_sq"):
                            if st and k in st:
                                dist.broadcast(st[k], dp.src0, group=dp.group)
        return same

    def _arange_p(self, p):
        t = getattr(self, "_arange_cache", None)
        if t is None or t.numel() != p:
            t = self._arange_cache = torch.arange(p, dtype=torch.int32, device=self.device)
        return t

    def _device_step(self, idx, cols, py):
        """minibatch gather + fused ELBO forward / backward (gradients land in ``.grad``); everything here is stream work"""
        dim, p, dev = self.dim, self.minibatch_dim, self.device
        nb = idx.shape[0]
        self.ctx.bind()                         # the library launches on torch's CURRENT stream (the capture stream under a graph)
        Db = None
        if self.X.dtype == torch.float64:       # fp64 model mode: dsvgp_gather_batch_f64 (x, interleaved y and the tiled directions, one launch)
            x_batch = torch.empty(nb, dim, dtype=torch.float64, device=dev)
            y_batch = torch.empty(nb * (py + 1), dtype=torch.float64, device=dev)
            fused_dirs = (not self.dfree and not self.full_gradient and py == p and p > 0
                          and self.E_canonical.shape == (dim, dim) and self.E_canonical.dtype == torch.float64
                          and self.E_canonical.is_contiguous())
            Db = torch.empty(nb * p, dim, dtype=torch.float64, device=dev) if fused_dirs else None
            _ops.gather_batch_f64(self.ctx, self.X, self.Y, idx, cols, py, x_batch, y_batch,
                                  self.E_canonical if fused_dirs else None, Db)
        else:
            x_batch = torch.empty(nb, dim, dtype=torch.float32, device=dev)
            y_batch = torch.empty(nb * (py + 1), dtype=torch.float32, device=dev)
            fused_dirs = (not self.dfree and not self.full_gradient and py == p and p > 0
                          and self.E_canonical.shape == (dim, dim) and self.E_canonical.dtype == torch.float32)
            Db = torch.empty(nb * p, dim, dtype=torch.float32, device=dev) if fused_dirs else None
            _ops.gather_batch(self.ctx, self.X, self.Y, idx, cols, py, x_batch, y_batch,  # interleaved y, :241
                              self.E_canonical if fused_dirs else None, Db)              # + the directions, :238
        kwargs = {}
        # (the directions are rows of E_canonical, the same p of them for every point: said to the engine as an index list next to
        #  the matrix itself -- _ops.state_directions -- so that K_ZX runs on the canonical-direction assembly kernels)
        if self.data_directions is not None:    # py canonical directions per point, py != the model's count: nothing to state
            kwargs["derivative_directions"] = self.E_canonical.index_select(0, cols[1:].long() - 1).repeat(nb, 1) if py else None
        elif self.dfree:                        # dfree_directional_vi.py:224-227
            kwargs["derivative_directions"] = _ops.state_directions(self.E_canonical[:p].repeat(nb, 1), self._arange_p(p), 0)
        elif not self.full_gradient:
            if Db is not None:
                kwargs["derivative_directions"] = _ops.state_directions(Db, cols[1:], 1)
            else:
                derivative_directions = self.E_canonical.index_select(0, cols[1:].long() - 1)
                kwargs["derivative_directions"] = _ops.state_directions(derivative_directions.repeat(nb, 1), cols[1:], 1)   # :238

        self.variational_optimizer.zero_grad()
        self.hyperparameter_optimizer.zero_grad()
        output = self.likelihood(self.model(x_batch, **kwargs))
        if self.autograd_protocol:
            loss = -self.mll(output, y_batch)           # the reference's three lines, through torch.autograd
            loss.backward()
        else:
            loss = self.mll.backward_step(output, y_batch)      # same numbers, gradients assigned directly
        return loss, output, y_batch

    # ---- HIP-graph replay of the steady-state step (launch-bound regimes: M' of a few hundred, per-rank shards) ----------
    # The whole device side of a step -- gather, assembly, Cholesky chain, solves, ELBO terms, backward, both Adam updates,
    # ~110 launches at M' = 600 -- is captured once per batch shape and replayed with ONE launch.  What varies per step
    # lives in device memory: the row indices and derivative columns (static buffers refreshed before the replay), the
    # learning rates and step counts of the two optimizers (pinned table + captured copy), the noise (the 2 vbar factor is
    # applied by the kernels, _step._elbo_fast).  The potrf status cannot be read inside a graph: the captured Adam kernels
    # are guarded by the status word, and the host looks at the status of step t before it launches step t + 1; a failed
    # factorisation (parameters untouched) is then redone eagerly through psd_safe_cholesky's jitter ladder.
    def _graph_eligible(self, need_variance):
        mode = self.graph
        if mode is None:
            env = os.environ.get("DSVGP_GRAPH")
            mode = None if env is None else env == "1"
        if mode is False or need_variance or self.dp is not None or self.autograd_protocol or self.data_directions is not None:
            return False
        eng = self.model.engine
        ok = (eng.whitening == "cholesky" and not eng.shared_directions and self.mll.mll_type == "ELBO"
              and isinstance(self.variational_optimizer, FusedAdam) and isinstance(self.hyperparameter_optimizer, FusedAdam)
              and eng.collective is None)
        if not ok:
            return False
        # opt-in only (``loop.graph = True`` / DSVGP_GRAPH=1 / ``bench.py --graph on``).  Measured on MI355X (round 2): the C2 step
        # (M' = 600, ~75 launches) is bound by its chain of DEPENDENT kernels (ten 24 us Cholesky launches, the fp64 products,
        # ~35 kernels at the few-us floor), which a graph replays at the same kernel-boundary cost: 0.74 ms replayed against
        # 0.77-0.80 ms eager at the end of round 2 (0.82-0.84 against 0.80 before the small products split K).
        return mode is True

    def _graph_step(self, idx, idx_y):
        # graph replay captures the piecewise path (its launches go to the capture stream one by one); the one-call step
        # (dsvgp_elbo_step_f32: its own second stream, a host read of the status word) is the alternative, not a part of it --
        # and the eager warm-up steps below must have created the piecewise path's buffers before the capture
        self.model.engine.c_step = False
        key = (idx.shape[0], len(idx_y))
        gs = self._graphs.get(key)
        if gs is None:
            seen = self._graph_seen[key] = self._graph_seen.get(key, 0) + 1
            if seen <= 2 or len(self._graphs) >= 2:        # eager warm-up (allocations, optimizer state); ragged tails stay eager
                self._graph_check_previous()
                return self._eager_step(idx, idx_y)
            self._graph_check_previous()
            gs = self._graphs[key] = self._capture(idx, idx_y)
        self._graph_check_previous()
        gs.idx.copy_(idx)
        gs.cols_host.copy_(torch.tensor(idx_y, dtype=torch.int32))
        for opt in (self.variational_optimizer, self.hyperparameter_optimizer):
            opt.fill_host_table()
        gs.graph.replay()
        gs.done.record()
        self._graph_pending = (gs, idx, list(idx_y))
        for opt, sch in ((self.variational_optimizer, self.variational_scheduler),
                         (self.hyperparameter_optimizer, self.hyperparameter_scheduler)):
            opt.advance_host_state()
            sch.step()
        return gs.loss, gs.output, gs.y_batch

    def _capture(self, idx, idx_y):
        import types
        dev, eng = self.device, self.model.engine
        gs = types.SimpleNamespace()
        gs.idx = idx.clone().contiguous()
        gs.cols_host = torch.tensor(idx_y, dtype=torch.int32).pin_memory()
        for opt in (self.variational_optimizer, self.hyperparameter_optimizer):
            opt.capture_tables(dev)
            opt.fill_host_table()
        torch.cuda.synchronize(dev)
        gs.graph = torch.cuda.CUDAGraph()
        guard = eng._buf["info"]                            # the potrf status word of the K_ZZ factorisation
        eng.capture_mode = True
        try:
            with torch.cuda.graph(gs.graph):
                cols = gs.cols_host.to(dev, non_blocking=True)
                gs.loss, gs.output, gs.y_batch = self._device_step(gs.idx, cols, len(idx_y) - 1)
                self.variational_optimizer.step_captured(guard)
                self.hyperparameter_optimizer.step_captured(guard)
        finally:
            eng.capture_mode = False
            self.ctx.bind()
        gs.done = torch.cuda.Event()
        gs.host_info = eng._host_info
        return gs

    def _graph_check_previous(self):
        """status of the previously replayed step (its Adam kernels did nothing if the factorisation failed)"""
        pend, self._graph_pending = self._graph_pending, None
        if pend is None:
            return
        gs, idx, idx_y = pend
        gs.done.synchronize()
        if int(gs.host_info[0]) == 0:
            return
        # K_ZZ + 1e-3 I was not positive definite in fp64: the parameters are untouched; redo the step eagerly (jitter
        # ladder of psd_safe_cholesky, NotPSDError after three tries) with the learning rates it was issued with
        opts = (self.variational_optimizer, self.hyperparameter_optimizer)
        lrs = [[g["lr"] for g in o.param_groups] for o in opts]
        for o in opts:
            for gi, g in enumerate(o.param_groups):
                g["lr"] = float(o._hp_host[gi, 0])
                for prm in g["params"]:
                    if o.state.get(prm):
                        o.state[prm]["step"] -= 1
        try:
            cols = torch.tensor(idx_y, dtype=torch.int32, device=self.device)
            self._device_step(idx.contiguous(), cols, len(idx_y) - 1)
            for o in opts:
                o.step()
        finally:
            for o, ls in zip(opts, lrs):
                for g, lr in zip(o.param_groups, ls):
                    g["lr"] = lr

    def refit_variational(self, minibatch_size=4096, data_directions=None, num_data=None, seed=None):
        """``fit_variational`` on the loop's resident (X, Y): q(u) <- the closed-form optimum for the current hyper-parameters and
        inducing set, with ``num_data`` the loop's own by default (the optimum of the objective the steps minimise).  The fused
        optimiser's moments (and step counts) of the tensors it overwrote start again from zero.  Returns the result object."""
        self.finish()
        if self.dp is not None:
            raise ValueError("refit_variational runs on one rank: a collective with world > 1 is not built for it")
        if num_data is None:
            num_data = self.mll.num_data
        result = fit_variational(self.model, self.likelihood, (self.X, self.Y), minibatch_size=minibatch_size,
                                 data_directions=data_directions, num_data=num_data, seed=seed)
        for prm in self.model.variational_parameters():
            st = self.variational_optimizer.state.get(prm)
            if st:
                st["step"] = 0
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
            prm.grad = None
        return result

    def set_missing_targets(self):
        """NaN entries of the resident targets are observations that do not exist from here on (``GPModel.missing_targets``; the engine's
        masked per-output step and collapsed statistics): Cholesky-whitened per-point model, float32, one rank -- anything else is refused.
        ``num_data`` of the objective becomes its value times the present fraction of Y, taken once here (one reduction, one host read)."""
        _enable_missing_targets(self)
        return self

    def set_derivative_noise(self):
        """The likelihood gets a second noise from here on (``GaussianLikelihood.add_derivative_noise``: ``raw_derivative_noise``, started
        at the value noise), registered with the hyper-parameter optimiser: function values are observed under ``likelihood.noise``,
        derivatives under ``likelihood.derivative_noise`` (the engine's two-class per-output step, predictions and collapsed statistics).
        Cholesky-whitened per-point model, float32, one rank, no missing targets, no graph replay -- anything else is refused."""
        _enable_derivative_noise(self)
        return self

    def finish(self):
        """drain the replay pipeline (the status of the last replayed / deferred step is checked here)"""
        self._graph_check_previous()
        self._deferred_check_previous()


def _kmeans_start(X, Y, num_inducing, num_directions, seed, dfree, shared):
    """(inducing points, inducing directions) of ``inducing_data_initialization="kmeans"`` (initialization.py): k-means centroids of X
    from a CPU generator seeded with ``seed``, and per point the leading eigenvectors of its cluster's gradient second moments
    (``Y[:, 1:]``); ``shared``: ONE direction set [p, d] from the moments of all gradients as one cluster; value-only targets (dfree)
    and inputs wider than the moment kernel keep canonical directions"""
    from . import initialization as _init
    gen = torch.Generator()
    if seed is not None:
        gen.manual_seed(int(seed))
    else:
        gen.seed()
    dim = X.shape[1]
    has_grad = (not dfree) and Y.dim() == 2 and Y.shape[1] == dim + 1 and dim <= _init.MOMENTS_MAX_DIM
    if shared:
        Z = _init.kmeans_inducing_points(X, num_inducing, generator=gen).centroids
        if has_grad:
            one = torch.zeros(X.shape[0], dtype=torch.int32, device=X.device)
            V = _init.gradient_directions(Y[:, 1:], one, 1, num_directions)
        else:
            V = torch.eye(dim)[:num_directions]
        return Z, V.to(X)
    return _init.initialize_inducing(X, Y if has_grad else None, num_inducing, num_directions, generator=gen)


def setup_training(train_dataset, num_inducing=128, num_directions=1, minibatch_size=1, minibatch_dim=1,
                   num_epochs=1, learning_rate_hypers=0.01, inducing_data_initialization=True, lr_sched=None,
                   mll_type="ELBO", gamma=0.1, fixed_inducing_locations=None, seed=None, tensors=None,
                   use_ngd=False, learning_rate_ngd=0.1, use_ciq=False, num_contour_quadrature=15, model_class=None,
                   dfree=False, shared=False, variational_initialization=None, data_directions=None, kernel="rbf",
                   ard_num_dims=None):
    """Everything ``train_gp`` does before its loop (directional_vi.py:130-219); returns a TrainLoop.
    NaN targets: ``TrainLoop.set_missing_targets()`` on the loop this returns (``train_gp(..., missing_targets=True)`` does that).
    ``inducing_data_initialization``: True (the first M data rows), False (uniform draws), or "kmeans" -- k-means centroids and gradient
    directions from the training tensors (``_kmeans_start``; one rank; ``fixed_inducing_locations`` wins over it).
    ``kernel`` ("rbf", the default, or "matern52"): the covariance family -- Matern-5/2 (scalar lengthscale, or ARD with
    ``ard_num_dims``) runs the engine's Matern step: Cholesky-whitened per-point model, float32, one rank.
    ``ard_num_dims`` (int, default None = one scalar lengthscale): one lengthscale per input dimension (must equal the input
    dimension) -- the engine's ARD step: Cholesky-whitened per-point model, float32, one rank.
    ``data_directions`` (int, default None = ``num_directions``): derivative columns of y per minibatch point, whatever the number of
    inducing directions (0: function values only; ``dim``: the full gradient) -- the engine's rectangular training step.
    ``variational_initialization`` (None, the default: q(u) = N(1e-3 randn, I) as the reference; or "optimal"): one
    ``TrainLoop.refit_variational`` before the first step -- q(u) starts at the closed-form optimum for the initial hyper-parameters."""
    assert num_directions == minibatch_dim
    if variational_initialization not in (None, "optimal"):
        raise ValueError("variational_initialization must be None or 'optimal', got %r" % (variational_initialization,))
    if isinstance(inducing_data_initialization, str):
        if inducing_data_initialization != "kmeans":
            raise ValueError("inducing_data_initialization must be True, False or 'kmeans', got %r" % (inducing_data_initialization,))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("inducing_data_initialization='kmeans' runs on one rank: the start is not replicated across a collective")
    if data_directions is not None:
        data_directions = int(data_directions)
        if dfree or shared or use_ciq:
            raise ValueError("data_directions is built for the Cholesky-whitened per-point DSVGP model (not dfree / shared / CIQ)")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("data_directions runs on one rank (dp): the rectangular training step is not built for a collective")
        if torch.get_default_dtype() == torch.float64 or (tensors is not None and tensors[0].dtype == torch.float64):
            raise ValueError("data_directions with a float64 dataset: the rectangular kernel backward is built in float32 only")
    if kernel not in ("rbf", "matern52"):
        raise ValueError("kernel must be 'rbf' or 'matern52', got %r" % (kernel,))
    if kernel == "matern52":
        if dfree or shared or use_ciq or use_ngd:
            raise ValueError("dfree / shared / CIQ / NGD training is not built for the Matern-5/2 kernel (kernel='matern52')")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("a collective with world > 1 is not built for the Matern-5/2 kernel (kernel='matern52')")
        if torch.get_default_dtype() == torch.float64 or (tensors is not None and tensors[0].dtype == torch.float64):
            raise ValueError("a float64 dataset is not built for the Matern-5/2 kernel (kernel='matern52'): the Matern kernels are float32")
    if ard_num_dims is not None:
        if dfree or shared or use_ciq or use_ngd:
            raise ValueError("dfree / shared / CIQ / NGD training is not built for ARD lengthscales (ard_num_dims)")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("a collective with world > 1 is not built for ARD lengthscales (ard_num_dims)")
        if torch.get_default_dtype() == torch.float64 or (tensors is not None and tensors[0].dtype == torch.float64):
            raise ValueError("a float64 dataset is not built for ARD lengthscales (ard_num_dims): the ARD kernels are float32")
    if not torch.cuda.is_available():
        raise RuntimeError("train_gp needs an MI355X (HIP) device: the DSVGP hot path has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    if tensors is not None:          # already-resident (X, Y)
        X, Y = tensors
    else:
        X, Y = _dataset_tensors(train_dataset, device)
    if Y.dim() == 1:                 # derivative-free data: scalar targets
        Y = Y.reshape(-1, 1).contiguous()
    model_class = model_class or GPModel
    n_samples, dim = X.shape
    num_data = (dim + 1) * n_samples                                      # :136

    if inducing_data_initialization == "kmeans" and fixed_inducing_locations is None:
        inducing_points, inducing_directions = _kmeans_start(X, Y, num_inducing, num_directions, seed, dfree, shared)
    else:
        if inducing_data_initialization is True:
            inducing_points = X[:num_inducing].clone()                        # first M data rows, :140-145
        else:
            inducing_points = torch.rand(num_inducing, dim).to(X)             # :149
        inducing_directions = torch.eye(dim)[:num_directions].repeat(num_inducing, 1).to(X)
        if shared and inducing_data_initialization is not True:          # shared_directional_vi.py:150-155: not tiled
            inducing_directions = torch.eye(dim)[:num_directions].to(X)

    learn_inducing_locations = True
    if fixed_inducing_locations is not None:
        inducing_points = fixed_inducing_locations.to(device)
        learn_inducing_locations = False

    if use_ciq:                                                           # :164-165
        model = model_class(inducing_points, inducing_directions, dim, variational_distribution="NGD",
                            variational_strategy="CIQ", learn_inducing_locations=learn_inducing_locations)
    elif use_ngd:                                                         # :166-167
        model = model_class(inducing_points, inducing_directions, dim, variational_distribution="NGD",
                            learn_inducing_locations=learn_inducing_locations)
    elif ard_num_dims is not None or kernel != "rbf":
        extra = {} if kernel == "rbf" else {"kernel": kernel}
        if ard_num_dims is not None:
            extra["ard_num_dims"] = int(ard_num_dims)
        model = model_class(inducing_points, inducing_directions, dim, learn_inducing_locations=learn_inducing_locations, **extra)
    else:
        model = model_class(inducing_points, inducing_directions, dim,
                            learn_inducing_locations=learn_inducing_locations)
    likelihood = GaussianLikelihood()
    model = model.to(X)                      # device and dtype of the data (fp64 model mode: see _step64)
    likelihood = likelihood.to(X)
    model.train()
    likelihood.train()

    dp = None
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dp = DataParallel()
        model.data_parallel = dp
    if seed is None and dp is not None:
        seed_t = torch.randint(0, 2 ** 31 - 1, (1,), device=device)
        dist.broadcast(seed_t, 0)
        seed = int(seed_t.item())
    col_rng = random.Random(seed) if seed is not None else random      # reference: global `random`
    perm_gen = torch.Generator(device=device)
    if seed is not None:
        perm_gen.manual_seed(seed)
    else:
        perm_gen.seed()
    if use_ciq:
        model.engine.ciq_num_quadrature = int(num_contour_quadrature)    # gpytorch.settings.num_contour_quadrature, :165
    model.variational_strategy._maybe_init()                              # q(u) <- N(0,I) + 1e-3 randn (first call)
    if dp is not None:   # identical initial state on every rank
        for t in model._param_list(likelihood):
            dist.broadcast(t.data, 0)

    if use_ngd or use_ciq:                                                # :186-187
        variational_optimizer = NGD(list(model.variational_parameters()), num_data=num_data, lr=learning_rate_ngd)
    else:
        variational_optimizer = make_adam([{"params": list(model.variational_parameters())}], lr=learning_rate_hypers)
    hyperparameter_optimizer = make_adam([
        {"params": list(model.hyperparameters())},
        {"params": list(likelihood.parameters())},
    ], lr=learning_rate_hypers)

    if lr_sched == "step_lr":
        num_batches = int(np.ceil(n_samples / minibatch_size))
        milestones = [int(num_epochs * num_batches / 3), int(2 * num_epochs * num_batches / 3)]
        hyperparameter_scheduler = torch.optim.lr_scheduler.MultiStepLR(hyperparameter_optimizer, milestones, gamma=gamma)
        variational_scheduler = torch.optim.lr_scheduler.MultiStepLR(variational_optimizer, milestones, gamma=gamma)
    else:
        if lr_sched is None:
            lr_sched = lambda epoch: 1.0
        hyperparameter_scheduler = torch.optim.lr_scheduler.LambdaLR(hyperparameter_optimizer, lr_lambda=lr_sched)
        variational_scheduler = torch.optim.lr_scheduler.LambdaLR(variational_optimizer, lr_lambda=lr_sched)

    if mll_type == "ELBO":
        mll = VariationalELBO(likelihood, model, num_data=num_data)
    elif mll_type == "PLL":
        mll = PredictiveLogLikelihood(likelihood, model, num_data=num_data)
    else:
        raise ValueError("mll_type must be 'ELBO' or 'PLL'")
    loop = TrainLoop(X, Y, model, likelihood, mll, (variational_optimizer, hyperparameter_optimizer),
                     (variational_scheduler, hyperparameter_scheduler), minibatch_dim, dp, col_rng, perm_gen, dfree=dfree)
    if data_directions is not None:
        if not 0 <= data_directions <= min(dim, 95) or Y.shape[1] != dim + 1:
            raise ValueError("data_directions must lie in [0, min(dim, 95)] = [0, %d] on targets with dim + 1 columns, got %d"
                             % (min(dim, 95), data_directions))
        if data_directions != num_directions:            # (equal counts: today's step, nothing to set)
            loop.data_directions = model.data_directions = data_directions
    if variational_initialization == "optimal":
        loop.refit_variational(data_directions=data_directions, seed=seed)
    return loop


def train_gp(train_dataset, num_inducing=128,
             num_directions=1, minibatch_size=1, minibatch_dim=1, num_epochs=1,
             learning_rate_hypers=0.01, learning_rate_ngd=0.1,
             inducing_data_initialization=True,
             use_ngd=False,
             use_ciq=False,
             lr_sched=None,
             mll_type="ELBO",
             num_contour_quadrature=15,
             watch_model=False, gamma=0.1,
             verbose=True,
             fixed_inducing_locations=None,
             data_directions=None,
             **args):
    """Train a Derivative GP with the Directional Derivative Variational Inference method
    (argument meaning identical to the reference, directional_vi.py:106-129).

    ``data_directions`` (int, not in the reference; default None = ``num_directions``): every minibatch carries that many derivative
    columns of y per point -- 0: function values only, ``dim``: the full gradient -- whatever the number of inducing directions.

    ``inducing_data_initialization="kmeans"`` (a value the reference does not have): k-means centroids of the inputs as inducing points
    and the leading eigenvectors of each cluster's gradient second moments as its directions (``setup_training``).

    Extra keyword arguments understood through ``**args`` (all optional, ignored by the reference):
      ``seed`` (int): seeds the minibatch permutation and the derivative-column sampling (must be equal
      on all ranks under torch.distributed; broadcast from rank 0 when omitted);
      ``max_steps`` (int): stop after this many optimisation steps;
      ``ard_num_dims`` (int, the input dimension): one lengthscale per input dimension (``setup_training``);
      ``kernel`` ("rbf" or "matern52"): the covariance family (``setup_training``);
      ``variational_initialization`` (None or "optimal"): start q(u) at its closed-form optimum (``setup_training``);
      ``missing_targets`` (bool): NaN entries of the targets are observations that do not exist (``TrainLoop.set_missing_targets``);
      ``derivative_noise`` (bool): one likelihood noise for the function values and one for the derivatives
      (``TrainLoop.set_derivative_noise``);
      ``loss_history`` (list): every step's loss is appended to it as a device scalar (no host read here).
    """
    assert num_directions == minibatch_dim
    missing = bool(args.get("missing_targets", False))
    two_noises = bool(args.get("derivative_noise", False))
    if two_noises and (missing or args.get("_shared") or args.get("_model_class") is not None):
        raise ValueError("derivative_noise is built for the per-point DSVGP harness (directional_vi.train_gp) without missing_targets, "
                         "not for the shared-directions harness or another model class")
    if two_noises and args.get("variational_initialization") not in (None, "optimal"):
        raise ValueError("variational_initialization must be None or 'optimal', got %r" % (args.get("variational_initialization"),))
    if missing and args.get("variational_initialization") not in (None, "optimal"):
        raise ValueError("variational_initialization must be None or 'optimal', got %r" % (args.get("variational_initialization"),))
    loop = setup_training(train_dataset, num_inducing, num_directions, minibatch_size, minibatch_dim, num_epochs,
                          learning_rate_hypers, inducing_data_initialization, lr_sched, mll_type, gamma,
                          fixed_inducing_locations, seed=args.get("seed"), use_ngd=use_ngd,
                          learning_rate_ngd=learning_rate_ngd, use_ciq=use_ciq,
                          num_contour_quadrature=num_contour_quadrature, model_class=args.get("_model_class"),
                          shared=bool(args.get("_shared")), data_directions=data_directions, kernel=args.get("kernel", "rbf"),
                          ard_num_dims=args.get("ard_num_dims"),
                          variational_initialization=None if missing or two_noises else args.get("variational_initialization"))
    if two_noises:                                           # (before the optimal start: it fits under both noises)
        loop.set_derivative_noise()
        if args.get("variational_initialization") == "optimal":
            loop.refit_variational(data_directions=data_directions, seed=args.get("seed"))
    if missing:                                              # (before any pass over the targets: the optimal start included)
        loop.set_missing_targets()
        if args.get("variational_initialization") == "optimal":
            loop.refit_variational(data_directions=data_directions, seed=args.get("seed"))
    n_samples = loop.X.shape[0]
    stride = (num_directions if loop.data_directions is None else loop.data_directions) + 1      # outputs per minibatch point
    max_steps = args.get("max_steps")
    history = args.get("loss_history")
    total_step = 0
    loss = None
    for i in range(num_epochs):
        perm = loop.epoch_permutation()
        for start in range(0, n_samples, minibatch_size):
            report = (total_step % 50 == 0) and verbose
            loss, output, y_batch = loop.step(perm[start:start + minibatch_size], need_variance="values" if report else False)
            if history is not None:
                history.append(loss.detach().clone())
            if report:
                means = output.mean[::stride]
                stds = output.value_variance.sqrt()          # = output.variance.sqrt()[::num_directions + 1]
                values = y_batch[::stride]
                if missing:                                  # the present function values only
                    ok = ~torch.isnan(values)
                    means, stds, values = means[ok], stds[ok], values[ok]
                nll = -torch.distributions.Normal(means, stds).log_prob(values).mean()
                print(f"Epoch: {i}; total_step: {total_step}, loss: {loss.item()}, nll: {nll}")
                sys.stdout.flush()
            total_step += 1
            if max_steps is not None and total_step >= max_steps:
                break
        if max_steps is not None and total_step >= max_steps:
            break

    loop.finish()
    if verbose and loss is not None:
        print(f"Done! loss: {loss.item()}")
        print("\nDone Training!")
    return loop.model, loop.likelihood


def _enable_missing_targets(loop):
    """``TrainLoop.set_missing_targets``: the refusals on the loop's switches alone, then the model's switch and the scaled ``num_data``"""
    model = loop.model
    no = lambda what: ValueError("missing_targets is built for the Cholesky-whitened per-point DSVGP model in float32 on one rank, not "
                                 "for %s" % what)
    if not isinstance(model, GPModel) or loop.dfree or getattr(loop, "plain", False) or loop.full_gradient:
        raise no("the dfree / shared / full-gradient / plain harnesses")
    eng = model.engine
    if eng.whitening != "cholesky" or eng.shared_directions or eng.data_outputs != "all":
        raise no("CIQ whitening, shared directions or derivative-free data")
    if isinstance(model.variational_strategy._variational_distribution, NaturalVariationalDistribution):
        raise no("natural parameters (NGD)")
    if loop.dp is not None:
        raise no("a collective with world > 1")
    if loop.X.dtype != torch.float32:
        raise no("a float64 dataset")
    if getattr(model, "missing_targets", False):
        return                                               # (already on: num_data was scaled then)
    model.missing_targets = True
    loop.mll.num_data = _present_num_data(loop.mll.num_data, loop.Y)


def _enable_derivative_noise(loop):
    """``TrainLoop.set_derivative_noise``: the refusals on the loop's switches alone, then the parameter and its optimiser group"""
    model, likelihood = loop.model, loop.likelihood
    no = lambda what: ValueError("derivative noise is built for the Cholesky-whitened per-point DSVGP model in float32 on one rank, "
                                 "not for %s" % what)
    if not isinstance(model, GPModel) or loop.dfree or getattr(loop, "plain", False) or loop.full_gradient:
        raise no("the dfree / shared / full-gradient / plain harnesses")
    eng = model.engine
    if eng.whitening != "cholesky" or eng.shared_directions or eng.data_outputs != "all":
        raise no("CIQ whitening, shared directions or derivative-free data")
    if isinstance(model.variational_strategy._variational_distribution, NaturalVariationalDistribution):
        raise no("natural parameters (NGD)")
    if loop.dp is not None:
        raise no("a collective with world > 1")
    if loop.X.dtype != torch.float32:
        raise no("a float64 dataset")
    if getattr(model, "missing_targets", False):
        raise no("missing_targets (one kernel carrying both is a follow-up)")
    if getattr(eng, "deterministic", False):
        raise no("the deterministic mode")
    if loop.graph is True or (loop.graph is None and os.environ.get("DSVGP_GRAPH") == "1"):
        raise no("graph replay of the step (capture_mode)")
    if not isinstance(likelihood, GaussianLikelihood):
        raise no("a likelihood other than GaussianLikelihood")
    if likelihood.has_derivative_noise:
        return                                               # (already there, e.g. built with derivative_noise=True)
    raw = likelihood.add_derivative_noise()
    # into the likelihood's own group (the last one) of the hyper-parameter optimiser: the schedulers were built on the groups as they
    # are, so the new parameter follows the learning rate of ``raw_noise``; its moments start with its first step
    loop.hyperparameter_optimizer.param_groups[-1]["params"].append(raw)


def _present_num_data(num_data, Y):
    """``num_data`` times the present (not NaN) fraction of the targets Y: one reduction, one host read"""
    return float(num_data) * float((~torch.isnan(Y)).sum().item()) / float(max(Y.numel(), 1))


def _default_num_data(model, X, Y, num_data):
    """the harness's own ``num_data``, (dim + 1) n_samples -- times the present fraction of Y for a model with ``missing_targets``"""
    if num_data is not None:
        return num_data
    n_samples, dim = X.shape
    num_data = (dim + 1) * n_samples
    return _present_num_data(num_data, Y) if getattr(model, "missing_targets", False) else num_data


def fit_variational(model, likelihood, dataset_or_tensors, minibatch_size=4096, data_directions=None, num_data=None, seed=None,
                    workspace_budget=1 << 30):
    """q(u) <- the maximiser of the ELBO over q(u) for the model's current hyper-parameters, inducing points and directions (Titsias
    2009; ``ElboEngine.collapsed_accumulator``), from ONE pass over the data in chunks of ``minibatch_size`` points.
    ``dataset_or_tensors``: a Dataset of (x[d], y[d+1]) pairs or resident (X, Y) tensors.  ``data_directions``: None -- the model's
    ``num_directions`` canonical derivative columns per chunk, drawn as ``select_cols_of_y`` draws them (from ``random.Random(seed)``, or
    the global ``random`` without a seed); an int -- that many; "all" -- the full gradient (d <= 95).  Scalar targets: values only.
    ``num_data`` defaults to the harness's own, (dim + 1) n_samples, so the optimum is that of the objective ``train_gp`` minimises.
    ``workspace_budget``: bytes of chunk workspace of the accumulator (a chunk of ``minibatch_size`` points is cut further to fit it).
    Writes (m*, L_S*) -- or (natural_vec, natural_mat) of a NaturalVariationalDistribution -- into the model and returns the result
    object (``variational_mean``, ``chol_variational_covar``, ``natural_vec``, ``natural_mat``, ``loss``, ``terms``)."""
    acc, X, Y, pd = _collapsed_setup(model, likelihood, dataset_or_tensors, data_directions, workspace_budget, "fit_variational")
    n_samples, dim = X.shape
    for x_batch, y_batch, D in _collapsed_chunks(X, Y, pd, minibatch_size, _collapsed_columns(n_samples, dim, pd, minibatch_size, seed)):
        acc.add(x_batch, y_batch, D)
    result = acc.solve(_default_num_data(model, X, Y, num_data))
    _write_variational(model, result)
    return result


def _collapsed_setup(model, likelihood, dataset_or_tensors, data_directions, workspace_budget, what):
    """(accumulator of the model's current state, resident X, Y [n, 1 or dim + 1], derivative columns per chunk) of one collapsed pass"""
    vs = model.variational_strategy
    device = vs.inducing_points.device
    if isinstance(dataset_or_tensors, (tuple, list)) and len(dataset_or_tensors) == 2 and torch.is_tensor(dataset_or_tensors[0]):
        X, Y = (t.to(device) for t in dataset_or_tensors)
    else:
        X, Y = _dataset_tensors(dataset_or_tensors, device, vs.inducing_points.dtype)
    if Y.dim() == 1:
        Y = Y.reshape(-1, 1)
    dim = X.shape[1]
    if hasattr(vs, "_maybe_init"):
        vs._maybe_init()                                  # (a later first training call must not re-initialise what is written here)
    acc = model.engine.collapsed_accumulator(model._param_dict(likelihood), workspace_budget=workspace_budget)
    if Y.shape[1] == 1:
        pd = 0
    elif data_directions is None:
        pd = int(model.num_directions)
    elif data_directions == "all":
        pd = dim
    else:
        pd = int(data_directions)
    if Y.shape[1] not in (1, dim + 1) or not 0 <= pd <= min(dim, 95) or (pd > 0 and Y.shape[1] == 1):
        raise ValueError("%s takes targets with 1 or dim + 1 = %d columns and 0 <= data_directions <= min(dim, 95) = %d, "
                         "got %d columns and %d directions" % (what, dim + 1, min(dim, 95), Y.shape[1], pd))
    return acc, X, Y, pd


def _collapsed_columns(n_samples, dim, pd, minibatch_size, seed):
    """the columns of y of every chunk of a pass, drawn as ``select_cols_of_y`` draws them (from ``random.Random(seed)``, or the global
    ``random`` without a seed): a list, so that a second pass over the same chunks takes the same columns"""
    rng = random.Random(seed) if seed is not None else random
    step = max(1, int(minibatch_size))
    return [list(range(dim + 1)) if pd == dim else sorted(rng.sample(range(1, dim + 1), pd) + [0]) for _ in range(0, n_samples, step)]


def _collapsed_chunks(X, Y, pd, minibatch_size, columns):
    """(x, interleaved y, canonical directions or None) of every chunk of ``minibatch_size`` points with its drawn columns"""
    dim = X.shape[1]
    E_canonical = torch.eye(dim, device=X.device, dtype=X.dtype)
    step = max(1, int(minibatch_size))
    for start, idx_y in zip(range(0, X.shape[0], step), columns):
        x_batch = X[start:start + step]
        y_batch = Y[start:start + step][:, idx_y].reshape(-1)
        D = E_canonical[[c - 1 for c in idx_y[1:]]].repeat(x_batch.shape[0], 1) if pd else None
        yield x_batch, y_batch, D


def _write_variational(model, result):
    """q(u) of the model <- the optimum: (m*, L_S*), or the natural pair of a NaturalVariationalDistribution"""
    vd = model.variational_strategy._variational_distribution
    with torch.no_grad():
        if isinstance(vd, NaturalVariationalDistribution):
            vd.natural_vec.copy_(result.natural_vec)
            vd.natural_mat.copy_(result.natural_mat)
        else:
            vd.variational_mean.copy_(result.variational_mean)
            vd.chol_variational_covar.copy_(result.chol_variational_covar)


def collapsed_loss_and_grads(model, likelihood, dataset_or_tensors, minibatch_size=4096, data_directions=None, num_data=None, seed=None,
                             workspace_budget=1 << 30, write_variational=True):
    """The collapsed bound (Titsias' SGPR objective: the ELBO with q(u) at its closed-form optimum) and its gradients with respect to
    the lengthscale(s), outputscale, noise, constant, inducing points and inducing directions, from TWO passes over the data in chunks
    of ``minibatch_size`` points: the statistics pass of ``fit_variational``, then ``CollapsedAccumulator.add_backward`` over the same
    chunks with the same drawn derivative columns.  Arguments as ``fit_variational``.  Fills ``.grad`` of the model's and the
    likelihood's hyper-parameters, the inducing points and the directions (those that require a gradient; added onto an existing
    ``.grad``); the variational tensors get none -- with ``write_variational`` they are set to the optimum itself.  Returns the result
    object of the solve (``loss``: the collapsed loss these gradients belong to)."""
    if getattr(likelihood, "has_derivative_noise", False):
        raise ValueError("derivative noise: the collapsed backward pass (collapsed_loss_and_grads, train_collapsed) is not built for two "
                         "noise classes -- d loss / d rho needs a per-class sum in the chunk pass (a follow-up); fit_variational is")
    acc, X, Y, pd = _collapsed_setup(model, likelihood, dataset_or_tensors, data_directions, workspace_budget, "collapsed_loss_and_grads")
    n_samples, dim = X.shape
    columns = _collapsed_columns(n_samples, dim, pd, minibatch_size, seed)
    for x_batch, y_batch, D in _collapsed_chunks(X, Y, pd, minibatch_size, columns):
        acc.add(x_batch, y_batch, D)
    result = acc.solve(_default_num_data(model, X, Y, num_data))
    acc.begin_backward(result)
    for x_batch, y_batch, D in _collapsed_chunks(X, Y, pd, minibatch_size, columns):
        acc.add_backward(x_batch, y_batch, D)
    _, grads = acc.finish_backward()
    if write_variational:
        _write_variational(model, result)
    for prm, name in zip(model._param_list(likelihood), model._param_names()):
        if name in grads and isinstance(prm, torch.nn.Parameter) and prm.requires_grad:
            g = grads[name].view_as(prm)
            prm.grad = g if prm.grad is None else prm.grad.add_(g)
    return result


def train_collapsed(train_dataset, num_inducing=128, num_directions=1, num_iterations=50, learning_rate_hypers=0.01, minibatch_size=4096,
                    data_directions=None, inducing_data_initialization=True, fixed_inducing_locations=None, kernel="rbf",
                    ard_num_dims=None, seed=None, num_data=None, workspace_budget=1 << 30, verbose=True, tensors=None,
                    missing_targets=False):
    """Train a derivative GP on its hyper-parameters, inducing points and inducing directions alone, with q(u) exact at every iterate
    (Titsias' SGPR for the directional-derivative model; RBF, ARD and Matern-5/2).  The model is built the way ``setup_training``
    builds it (``kernel``, ``ard_num_dims``, ``inducing_data_initialization``, ``fixed_inducing_locations``, ``seed`` and ``verbose``
    as ``train_gp`` understands them; ``missing_targets``: NaN targets do not exist); each of the ``num_iterations`` iterations is one ``collapsed_loss_and_grads`` over the whole data
    set -- chunks of ``minibatch_size`` points, derivative columns drawn once per iteration -- and one Adam step at
    ``learning_rate_hypers``; a final ``fit_variational`` leaves q(u) at the optimum of the final hyper-parameters.
    Returns (model, likelihood)."""
    loop = setup_training(train_dataset, num_inducing, num_directions, minibatch_size, num_directions, 1, learning_rate_hypers,
                          inducing_data_initialization, None, "ELBO", 0.1, fixed_inducing_locations, seed=seed, tensors=tensors,
                          data_directions=data_directions, kernel=kernel, ard_num_dims=ard_num_dims)
    model, likelihood = loop.model, loop.likelihood
    if missing_targets:
        loop.set_missing_targets()
        if num_data is None:
            num_data = loop.mll.num_data                 # the present fraction was taken once, there
    optimizer = loop.hyperparameter_optimizer
    rng = random.Random(seed) if seed is not None else random
    pass_seed = lambda: rng.randrange(2 ** 31)
    result = None
    for it in range(int(num_iterations)):
        for prm in list(model.parameters()) + list(likelihood.parameters()):
            prm.grad = None
        result = collapsed_loss_and_grads(model, likelihood, (loop.X, loop.Y), minibatch_size=minibatch_size, data_directions=data_directions,
                                          num_data=num_data, seed=pass_seed(), workspace_budget=workspace_budget, write_variational=False)
        optimizer.step()
        if verbose and it % 10 == 0:
            print(f"Iteration: {it}; collapsed loss: {result.loss}")
            sys.stdout.flush()
    fit_variational(model, likelihood, (loop.X, loop.Y), minibatch_size=minibatch_size, data_directions=data_directions, num_data=num_data,
                    seed=pass_seed(), workspace_budget=workspace_budget)
    if verbose and result is not None:
        print(f"Done! collapsed loss: {result.loss}")
    return model, likelihood


def eval_gp(test_dataset, model, likelihood,
            mll_type="ELBO", num_directions=1, minibatch_size=1, minibatch_dim=1):
    """Predictive means / variances (with likelihood noise) of all (p+1) outputs per test point,
    returned as CPU vectors of length N_test*(p+1), interleaved (reference directional_vi.py:271-305)."""
    assert num_directions == minibatch_dim
    dim = len(test_dataset[0][0])
    device = model.variational_strategy.inducing_points.device
    X, _ = _dataset_tensors(test_dataset, device, model.variational_strategy.inducing_points.dtype)
    n_test = X.shape[0]

    model.eval()
    likelihood.eval()

    means = []
    variances = []
    with torch.no_grad():
        for start in range(0, n_test, minibatch_size):
            x_batch = X[start:start + minibatch_size]
            # redo derivative directions b/c batch size is not consistent
            derivative_directions = torch.eye(dim, device=device)[:num_directions]
            derivative_directions = derivative_directions.repeat(len(x_batch), 1)
            if derivative_directions.is_cuda:   # eye(d)[:p] tiled: one-hot and shared (canonical-direction assembly)
                _ops.state_directions(derivative_directions, torch.arange(num_directions, dtype=torch.int32, device=device), 0)
            preds = likelihood(model(x_batch, derivative_directions=derivative_directions))
            means.append(preds.mean.cpu())
            variances.append(preds.variance.cpu())
    means = torch.cat(means) if means else torch.zeros(0)
    variances = torch.cat(variances) if variances else torch.zeros(0)
    print("Done Testing!")
    return means, variances


def eval_mean(test_dataset, model, num_directions=1, minibatch_size=1, minibatch_dim=1):
    """``eval_gp(...)[0]`` for callers that read only the means (reference experiments/bunny/exp_bunny.py:189-195
    ``means, _ = eval_gp(...)``): same batching, the same ``eye(d)[:p]`` directions, same ordering, CPU vector of length
    N_test*(p+1) -- through ``model.posterior_mean`` (no K_ZX, no solve, no variances)."""
    assert num_directions == minibatch_dim
    dim = len(test_dataset[0][0])
    device = model.variational_strategy.inducing_points.device
    X, _ = _dataset_tensors(test_dataset, device, model.variational_strategy.inducing_points.dtype)
    n_test = X.shape[0]

    model.eval()

    means = []
    with torch.no_grad():
        for start in range(0, n_test, minibatch_size):
            x_batch = X[start:start + minibatch_size]
            derivative_directions = torch.eye(dim, device=device)[:num_directions]
            derivative_directions = derivative_directions.repeat(len(x_batch), 1)
            means.append(model.posterior_mean(x_batch, derivative_directions=derivative_directions).cpu())
    return torch.cat(means) if means else torch.zeros(0)


def eval_paths(dataset_or_tensor, paths, minibatch_size, gradients=False):
    """Posterior function draws (``model.sample_paths(...)``) over a whole dataset (its x) or a tensor [N, d], in minibatches: the values
    [n, N] concatenated ON THE DEVICE and, with ``gradients=True``, also the gradients [n, N, d].  The same functions in every
    batch: for d <= 32 the result does not depend on ``minibatch_size``."""
    if torch.is_tensor(dataset_or_tensor):
        X = dataset_or_tensor.to(device=paths.device, dtype=torch.float32)
        if X.dim() == 1:
            X = X.unsqueeze(-1)
    else:
        X, _ = _dataset_tensors(dataset_or_tensor, paths.device, torch.float32)
    minibatch_size = max(int(minibatch_size), 1)
    vals, grads = [], []
    for start in range(0, X.shape[0], minibatch_size):
        xb = X[start:start + minibatch_size]
        if gradients:
            v, g = paths.values_and_gradients(xb)
            grads.append(g)
        else:
            v = paths.values(xb)
        vals.append(v)
    if not vals:
        raise ValueError("eval_paths needs at least one point")
    values = torch.cat(vals, dim=1)
    return (values, torch.cat(grads, dim=1)) if gradients else values


def thompson_candidates(paths, candidates, lower, upper, num_starts=8, iterations=20, maximize=False):
    """One Thompson step with refinement: every path (``model.sample_paths(...)``) is evaluated at the shared ``candidates`` [N, d]
    (``paths.values``), its ``num_starts`` best candidates become its own starts [n, num_starts, d], ``paths.descend`` refines each
    start ON ITS OWN PATH inside the box [lower, upper] ([d] each) and the best refined start per path is returned:
    (x_next [n, d], f_next [n], f_candidates_best [n]) with f_next never worse than f_candidates_best, the path's best value over
    the candidates (what the reference's TuRBO loops stop at: the arg-min of each joint draw)."""
    X = candidates.to(device=paths.device, dtype=torch.float32)
    if X.dim() == 1:
        X = X.unsqueeze(-1)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] != paths.d:
        raise ValueError("candidates must be [N, d] = [N >= 1, %d], got %s" % (paths.d, tuple(X.shape)))
    k = max(1, min(int(num_starts), X.shape[0]))
    vals = paths.values(X)                                              # [n, N]: the shared-point kernel
    top = torch.topk(vals, k, dim=1, largest=bool(maximize))
    starts = X[top.indices]                                             # [n, k, d]
    res = paths.descend(starts, lower.to(paths.device), upper.to(paths.device), iterations=iterations, maximize=maximize)
    best = res.values.argmax(dim=1) if maximize else res.values.argmin(dim=1)
    rows = torch.arange(res.x.shape[0], device=paths.device)
    return res.x[rows, best], res.values[rows, best], top.values[:, 0]


def acquisition_candidates(predictor, candidates, lower, upper, kind="lcb", beta=2.0, best=None, maximize=False, num_starts=8,
                           iterations=20):
    """One confidence-bound / expected-improvement step with refinement, in the pattern of ``thompson_candidates``: the acquisition
    ``kind`` of ``predictor`` (``model._variance_predictor()`` / ``ElboEngine.variance_predictor``; smaller is better) is evaluated
    at the ``candidates`` [N, d], its ``num_starts`` best become the starts of ``predictor.descend`` inside the box [lower, upper]
    ([d] each) and the best refined start is returned: (x_next [d], a_next, a_candidates_best) with a_next never worse than
    a_candidates_best, the best acquisition value over the candidates (where the reference's loops stop: the arg-min of
    ``preds.mean - lcb_beta * preds.variance``, experiments/rover/bo_traditional.py:214)."""
    X = candidates.to(device=predictor.device, dtype=torch.float32)
    if X.dim() == 1:
        X = X.unsqueeze(-1)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] != predictor.d:
        raise ValueError("candidates must be [N, d] = [N >= 1, %d], got %s" % (predictor.d, tuple(X.shape)))
    k = max(1, min(int(num_starts), X.shape[0]))
    lower, upper = lower.to(predictor.device), upper.to(predictor.device)
    vals = predictor.acquisition(X, kind, beta, best, maximize)          # [N]
    top = torch.topk(vals, k, largest=False)
    # (a start outside the box is clamped by the descent, which may raise its value: the candidates' best stays in the comparison)
    res = predictor.descend(X[top.indices], lower, upper, kind, beta, best, maximize, iterations=iterations)
    i = res.values.argmin()
    a_best = top.values[0]
    take = res.values[i] <= a_best
    x_next = torch.where(take, res.x[i], X[top.indices[0]])
    return x_next, torch.where(take, res.values[i], a_best), a_best


def eval_values(test_dataset, model, likelihood, minibatch_size=1):
    """``eval_gp(...)`` followed by ``[::p+1]``: predictive means / variances (with likelihood noise) of the FUNCTION VALUES,
    what the reference's callers keep of it (tests/test_dsvgp.py:99-101, the experiments' MSE / NLL reports).  Same batching and
    noise handling as ``eval_gp``, CPU vectors of length N_test -- through ``model.posterior(x)``: K_ZX, the solve and W are
    formed for B columns per batch instead of B(p+1)."""
    device = model.variational_strategy.inducing_points.device
    X, _ = _dataset_tensors(test_dataset, device, model.variational_strategy.inducing_points.dtype)
    n_test = X.shape[0]

    model.eval()
    likelihood.eval()

    means = []
    variances = []
    with torch.no_grad():
        for start in range(0, n_test, minibatch_size):
            preds = model.posterior(X[start:start + minibatch_size], likelihood=likelihood)
            means.append(preds.mean.cpu())
            variances.append(preds.variance.cpu())
    means = torch.cat(means) if means else torch.zeros(0)
    variances = torch.cat(variances) if variances else torch.zeros(0)
    return means, variances


def eval_gradients(test_dataset, model, likelihood, minibatch_size=1):
    """Value and full gradient of f at every test point WITH their joint uncertainty: ``model.posterior_gradient`` over the
    dataset in the batches of ``eval_values``.  Returns its named tuple -- value_mean [N], value_variance [N], gradient_mean
    [N, d], gradient_covariance [N, d, d], value_gradient_covariance [N, d] (with likelihood noise on the variances) --
    concatenated ON THE DEVICE: N d^2 floats stay where the caller's next step (descent probabilities, normal cones,
    gradient-norm bounds) runs.  Whatever number of directions the model was trained with; d <= 95."""
    device = model.variational_strategy.inducing_points.device
    X, _ = _dataset_tensors(test_dataset, device, model.variational_strategy.inducing_points.dtype)
    n_test = X.shape[0]

    model.eval()
    likelihood.eval()

    parts = []
    with torch.no_grad():
        for start in range(0, n_test, minibatch_size):
            parts.append(model.posterior_gradient(X[start:start + minibatch_size], likelihood=likelihood))
    if not parts:
        raise ValueError("eval_gradients needs at least one test point")
    return type(parts[0])(*[torch.cat(field) for field in zip(*parts)])


GradientNLL = collections.namedtuple("GradientNLL", ["nll", "whitened", "value_nll"])


def eval_gradient_nll(test_dataset, model, likelihood, minibatch_size=1):
    """How well the model predicts the gradient JOINTLY with the value: for a test set whose ``y`` carries [f, grad f] (d + 1
    columns, as the reference's datasets do), a named tuple, concatenated ON THE DEVICE, of
    nll [N]: minus the joint log-density of [f, grad f] at every point under the likelihood (``model.gradient_log_prob``);
    whitened [N, d + 1]: L^-1 (y - mean) with L the root of the point's covariance block -- standard normal if the joint
    uncertainty is calibrated; value_nll [N]: the same for the function value alone (the q = 1 marginal), the per-point form of
    the NLL the reference's harness prints.  Points are scored one by one, in the batches of ``eval_gradients``: nothing of size
    B (d + 1) squared is formed.  Whatever number of directions the model was trained with; d <= 95."""
    device = model.variational_strategy.inducing_points.device
    X, Y = _dataset_tensors(test_dataset, device, model.variational_strategy.inducing_points.dtype)
    n_test, d = X.shape
    if Y.dim() != 2 or Y.shape[1] != d + 1:
        raise ValueError("eval_gradient_nll needs y = [f, grad f] with d + 1 = %d columns, got %s" % (d + 1, tuple(Y.shape)))
    if d > 95:
        raise ValueError("eval_gradient_nll takes all d partial derivatives as data directions: at most 95, got d = %d" % d)
    if n_test == 0:
        raise ValueError("eval_gradient_nll needs at least one test point")

    model.eval()
    likelihood.eval()

    nll, whitened, value_nll = [], [], []
    with torch.no_grad():
        for start in range(0, n_test, minibatch_size):
            x, y = X[start:start + minibatch_size], Y[start:start + minibatch_size]
            B = x.shape[0]
            post = model.posterior(x, torch.eye(d, dtype=x.dtype, device=device).repeat(B, 1), likelihood)
            z, logp = post._point_density(y)
            # the value alone: the [0, 0] entries as B blocks of 1 x 1 through the same kernels
            engine = model.engine
            roots1, logdet1 = engine.block_roots(post.point_covariances[:, :1, :1].contiguous())
            _, logp1 = engine.block_log_prob(post.mean.reshape(B, d + 1)[:, 0].contiguous(), roots1, logdet1,
                                             y[:, 0].to(torch.float32).contiguous())
            nll.append(-logp)
            whitened.append(z)
            value_nll.append(-logp1)
    return GradientNLL(torch.cat(nll), torch.cat(whitened), torch.cat(value_nll))
