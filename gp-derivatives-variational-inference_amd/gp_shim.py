"""Minimal host-side stand-ins for the GPyTorch 1.4.0 objects the reference's hot path touches.

gpytorch is a third-party dependency of the reference (graphite_environment.yml:101) and is not
available here; these classes keep the parameter names / shapes / state_dict keys and the call
protocol (``model(x, derivative_directions=D)`` -> distribution, ``likelihood(dist)``,
``mll(output, y)``) that ``directional_vi.train_gp`` relies on (directional_vi.py:25-65,172,216-219,245-246),
and route the arithmetic to the HIP engine (``_step.ElboEngine``).  They contain no math of their own.
"""
import collections

import torch

from . import _ops
from ._step import ElboEngine, NGD_PARAM_NAMES, PARAM_NAMES


class OldVersionWarning(UserWarning):
    """gpytorch.utils.warnings.OldVersionWarning: a checkpoint written before the whitened VariationalStrategy was loaded"""


class PriorDistribution:
    """``strategy(x, prior=True)``: the un-whitened prior p(u) at the inducing points (``.loc``, ``.covariance_matrix``)"""

    def __init__(self, loc, covariance_matrix):
        self.loc = self.mean = loc
        self.covariance_matrix = covariance_matrix


class ConstantMean(torch.nn.Module):
    """gpytorch.means.ConstantMean: parameter ``constant`` of shape [1], init 0."""

    def __init__(self):
        super().__init__()
        self.register_parameter("constant", torch.nn.Parameter(torch.zeros(1)))


class ScaleKernel(torch.nn.Module):
    """gpytorch.kernels.ScaleKernel: ``raw_outputscale`` (0-dim, softplus-constrained, init 0)."""

    def __init__(self, base_kernel):
        super().__init__()
        self.base_kernel = base_kernel
        self.register_parameter("raw_outputscale", torch.nn.Parameter(torch.zeros(())))

    @property
    def outputscale(self):
        return torch.nn.functional.softplus(self.raw_outputscale)


class _NoiseCovar(torch.nn.Module):
    def __init__(self, derivative_noise=False):
        super().__init__()
        self.register_parameter("raw_noise", torch.nn.Parameter(torch.zeros(1)))
        if derivative_noise:
            self.register_parameter("raw_derivative_noise", torch.nn.Parameter(torch.zeros(1)))


class GaussianLikelihood(torch.nn.Module):
    """gpytorch.likelihoods.GaussianLikelihood: ``noise_covar.raw_noise`` [1], noise = softplus + 1e-4.
    ``derivative_noise=True`` (not in gpytorch's class; its derivative-GP examples use one noise per output of [f, grad f]): a second
    parameter ``noise_covar.raw_derivative_noise`` [1] under the same constraint -- the function-value rows are then observed under
    ``noise``, the directional-derivative rows under ``derivative_noise`` (csrc/noise_classes.hip).  The default's state_dict is as before."""

    def __init__(self, derivative_noise=False):
        super().__init__()
        self.noise_covar = _NoiseCovar(bool(derivative_noise))

    @property
    def has_derivative_noise(self):
        return "raw_derivative_noise" in self.noise_covar._parameters

    def add_derivative_noise(self):
        """register ``noise_covar.raw_derivative_noise`` at the current value of ``raw_noise`` (nothing if it is there); returns it"""
        if not self.has_derivative_noise:
            raw = self.noise_covar.raw_noise
            self.noise_covar.register_parameter("raw_derivative_noise", torch.nn.Parameter(raw.detach().clone()))
        return self.noise_covar.raw_derivative_noise

    @property
    def noise(self):
        return torch.nn.functional.softplus(self.noise_covar.raw_noise) + 1e-4

    @property
    def derivative_noise(self):
        if not self.has_derivative_noise:
            raise AttributeError("this likelihood has one noise: GaussianLikelihood(derivative_noise=True) has a second")
        return torch.nn.functional.softplus(self.noise_covar.raw_derivative_noise) + 1e-4

    def forward(self, dist):
        return dist.with_likelihood(self)


def _param_names(model, likelihood):
    """the model's parameter names; a likelihood with a derivative noise is handed over (``GPModel`` appends its name)"""
    return model._param_names(likelihood) if getattr(likelihood, "has_derivative_noise", False) else model._param_names()


def _noise_rows(params, q):
    """the likelihood noise of the q = pd + 1 rows of a point as the engine added it: [q] with the derivative noise on rows 1.., or a
    0-dim tensor for a single noise (a model's ``_param_dict(None)`` carries the stand-in noise alone)"""
    soft = torch.nn.functional.softplus
    n_f = soft(params["raw_noise"].reshape(())) + 1e-4
    if "raw_derivative_noise" not in params:
        return n_f
    out = n_f.reshape(1).repeat(q)
    out[1:] = soft(params["raw_derivative_noise"].reshape(())) + 1e-4
    return out


class _VariationalDistribution(torch.nn.Module):
    pass


class CholeskyVariationalDistribution(_VariationalDistribution):
    """gpytorch.variational.CholeskyVariationalDistribution: mean zeros, Cholesky factor identity."""

    def __init__(self, num_inducing_points, mean_init_std=1e-3):
        super().__init__()
        self.mean_init_std = mean_init_std
        self.register_parameter("variational_mean", torch.nn.Parameter(torch.zeros(num_inducing_points)))
        self.register_parameter("chol_variational_covar", torch.nn.Parameter(torch.eye(num_inducing_points)))
        # (only the lower triangle is a parameter -- forward() masks the rest, its gradient is exactly zero there: optim.FusedAdam then
        #  walks the lower triangle only, half the traffic of the update's largest tensor)
        self.chol_variational_covar._dsvgp_tril = True

    def initialize_variational_distribution(self):
        """prior N(0, I): mean <- 0 + mean_init_std * randn, chol <- I (first training call in gpytorch)."""
        with torch.no_grad():
            self.variational_mean.zero_()
            self.variational_mean.add_(torch.randn_like(self.variational_mean), alpha=self.mean_init_std)
            self.chol_variational_covar.copy_(torch.eye(self.variational_mean.shape[0],
                                                        device=self.variational_mean.device))


class NaturalVariationalDistribution(_VariationalDistribution):
    """gpytorch.variational.NaturalVariationalDistribution (1.4.0): q(u) = N(m, S) held in natural parameters
    ``natural_vec`` = S^-1 m (init 0) and ``natural_mat`` = -S^-1 / 2 (init -I/2).  The gradients the engine returns
    for them are taken w.r.t. the expectation parameters, so ``optim.NGD`` performs natural gradient descent
    (reference directional_vi.py:35-37,186-187)."""

    def __init__(self, num_inducing_points, mean_init_std=1e-3):
        super().__init__()
        self.mean_init_std = mean_init_std
        self.register_parameter("natural_vec", torch.nn.Parameter(torch.zeros(num_inducing_points)))
        self.register_parameter("natural_mat", torch.nn.Parameter(torch.eye(num_inducing_points).mul_(-0.5)))

    def initialize_variational_distribution(self):
        """prior N(0, I): natural_vec <- P 0 + mean_init_std * randn, natural_mat <- -P / 2 with P = I."""
        with torch.no_grad():
            self.natural_vec.zero_()
            self.natural_vec.add_(torch.randn_like(self.natural_vec), alpha=self.mean_init_std)
            self.natural_mat.copy_(torch.eye(self.natural_vec.shape[0], device=self.natural_vec.device).mul_(-0.5))


class _ElboFunction(torch.autograd.Function):
    """Fused forward+backward of one minibatch objective on the HIP engine."""

    @staticmethod
    def forward(ctx, engine, x, y, D, num_data, mll_type, dp, names, *params):
        pd = dict(zip(names, [_ops.detach_keep(p) for p in params]))
        if dp is not None:
            loss, grads, mu, varn = dp.loss_and_grads(engine, pd, x, y, D, num_data, mll_type)
        else:
            loss, grads, mu, varn = engine.loss_and_grads(pd, x, y, D, num_data, mll_type)
        ctx.grads = [grads[k] for k in names]
        ctx.mark_non_differentiable(mu, varn)
        return -loss, mu, varn          # mll value = -loss

    @staticmethod
    def backward(ctx, g_elbo, _gm, _gv):
        # d loss / d param = -(d loss / d mll) * grads; the engine's buffers are consumed in place (multi-tensor
        # scale by the device scalar: no per-parameter temporaries, the 36 MB L_S gradient is not copied)
        grads = ctx.grads
        ctx.grads = None
        torch._foreach_mul_(grads, -g_elbo.detach().to(grads[0].dtype))
        return tuple([None] * 8 + list(grads))


PosteriorGradient = collections.namedtuple("PosteriorGradient", ["value_mean", "value_variance", "gradient_mean", "gradient_covariance",
                                                                 "value_gradient_covariance"])


class PredictiveDistribution:
    """What ``model(x, derivative_directions=D)`` returns: a handle whose ``mean`` / ``variance``
    (length B(p+1), interleaved) are produced on the GPU on demand."""

    def __init__(self, model, x, D, likelihood=None):
        self.model, self.x, self.D, self.likelihood = model, x, D, likelihood
        self._mu = self._varn = self._var = None

    def with_likelihood(self, likelihood):
        out = PredictiveDistribution(self.model, self.x, self.D, likelihood)
        return out

    def _ensure(self):
        if self._mu is None or self._varn is None:
            lik = self.likelihood
            params = self.model._param_dict(lik)
            mu, varn = self.model.engine.predict(params, self.x, self.D, cache=not self.model.training)
            self._mu, self._varn = mu, varn
            if lik is None:   # q(f) itself: remove the noise again
                if "raw_derivative_noise" in params:
                    q = varn.numel() // max(self.x.shape[0], 1)
                    self._var = (varn.view(-1, q) - _noise_rows(params, q)).reshape(-1)
                else:
                    self._var = (varn - torch.nn.functional.softplus(params["raw_noise"].reshape(())) - 1e-4)

    @property
    def mean(self):
        if self._mu is None:        # (a fast-path training step has left its mean here; only the variance is then on demand)
            self._ensure()
        return self._mu

    loc = mean

    @property
    def variance(self):
        self._ensure()
        return self._varn if self.likelihood is not None else self._var

    @property
    def value_variance(self):
        """``variance[::p+1]`` (the function-value rows).  After a training step taken with ``need_variance="values"`` it is
        the vector the engine formed from that step's own forward pass (ElboEngine.value_variances); otherwise a slice."""
        v = getattr(self, "_value_varn", None)
        if v is not None and self.likelihood is not None:
            return v
        return self.variance[::getattr(self, "_value_stride", 1)]

    @property
    def stddev(self):
        return self.variance.sqrt()

    def confidence_region(self):
        """(mean - 2 std, mean + 2 std), gpytorch MultivariateNormal.confidence_region"""
        std2 = self.stddev.mul(2)
        return self.mean - std2, self.mean + std2

    # ---- joint distribution over the B(p+1) outputs of the batch (BO drivers: ``preds.sample(torch.Size([n]))``,
    #      reference experiments/GNN_bo/gcn_turbo.py:238-239, experiments/rover/test_turbo.py:138) ----
    def _ensure_joint(self):
        if getattr(self, "_Sigma", None) is None:
            lik = self.likelihood
            params = self.model._param_dict(lik)
            mu, Sigma = self.model.engine.predict_joint(params, self.x, self.D, cache=not self.model.training)
            if lik is None:   # q(f) itself: remove the noise again
                if "raw_derivative_noise" in params:
                    q = Sigma.shape[0] // max(self.x.shape[0], 1)
                    Sigma.diagonal().view(-1, q).sub_(_noise_rows(params, q))
                else:
                    Sigma.diagonal().sub_(torch.nn.functional.softplus(params["raw_noise"].reshape(())) + 1e-4)
            self._mu, self._Sigma, self._root = mu, Sigma, None

    @property
    def covariance_matrix(self):
        self._ensure_joint()
        return self._Sigma

    @property
    def point_covariances(self):
        """[B, pd + 1, pd + 1]: the covariance of (f(x), D_1 f(x), ..., D_pd f(x)) at every point of the batch -- the diagonal
        blocks of ``covariance_matrix`` without forming it (``ElboEngine.predict_blocks``: nothing of size B' x B').  With the
        likelihood's noise on the block diagonals when the distribution carries a likelihood, q(f) itself otherwise."""
        if getattr(self, "_blocks", None) is None:
            lik = self.likelihood
            params = self.model._param_dict(lik)
            mu, blocks = self.model.engine.predict_blocks(params, self.x, self.D, cache=not self.model.training)
            if lik is None:   # q(f) itself: remove the noise again
                blocks.diagonal(dim1=1, dim2=2).sub_(_noise_rows(params, blocks.shape[-1]))
            self._mu, self._blocks = mu, blocks
        return self._blocks

    @property
    def point_roots(self):
        """(roots f64 [B, pd + 1, pd + 1], logdet f64 [B]): the lower Cholesky factor and the log-determinant of every block of
        ``point_covariances`` (with the noise when the distribution carries a likelihood, q(f) otherwise), factorised in fp64 on
        the GPU with the jitter ladder of ``rsample``'s root (``ElboEngine.block_roots``).  Formed once per distribution."""
        if getattr(self, "_point_roots", None) is None:
            self._point_roots = self.model.engine.block_roots(self.point_covariances)
        return self._point_roots

    def rsample_points(self, sample_shape=torch.Size(), base_samples=None):
        """mean + L_b eps_b at every point b, L_b the root of the point's block (``point_roots``): draws of
        (f(x), D_1 f(x), ..., D_pd f(x)) that are EXACT WITHIN a point and INDEPENDENT BETWEEN points -- nothing of size
        B' x B' is formed.  ``sample`` / ``rsample`` are the jointly correlated form (and pay for the whole covariance).  Shape
        ``sample_shape + [B(pd+1)]``, in the interleaved order of ``sample``; ``base_samples`` (that many standard normal numbers)
        replaces ``torch.randn`` on the device."""
        roots, _ = self.point_roots
        mu = self._mu
        n_out = mu.shape[0]
        sample_shape = torch.Size(sample_shape)
        n = int(sample_shape.numel()) if len(sample_shape) else 1
        if base_samples is None:
            eps = torch.randn(n, n_out, dtype=torch.float32, device=mu.device)
        else:
            eps = base_samples.to(device=mu.device, dtype=torch.float32).reshape(n, n_out).contiguous()
        return self.model.engine.block_draw(mu, roots, eps).reshape(tuple(sample_shape) + (n_out,))

    def sample_points(self, sample_shape=torch.Size(), base_samples=None):
        """``rsample_points`` without a graph: per-point draws, independent between points (``sample``: jointly correlated)"""
        with torch.no_grad():
            return self.rsample_points(sample_shape, base_samples)

    def _point_density(self, y):
        roots, logdet = self.point_roots
        mu = self._mu
        y = y.to(device=mu.device, dtype=torch.float32).reshape(-1).contiguous()
        if y.numel() != mu.numel():
            raise ValueError("y has %d entries, the distribution B (pd + 1) = %d" % (y.numel(), mu.numel()))
        return self.model.engine.block_log_prob(mu, roots, logdet, y)

    def point_log_prob(self, y):
        """[B]: the joint log-density of (y_b0, ..., y_b,pd) under N(mean_b, point_covariances[b]) at every point; ``y`` has
        B (pd + 1) entries, interleaved or as [B, pd + 1].  Points are scored one by one: no correlation between points enters."""
        return self._point_density(y)[1]

    def point_whitened_residuals(self, y):
        """[B, pd + 1]: L_b^-1 (y_b - mean_b) with L_b the root of the point's block -- standard normal entries if the joint
        uncertainty of value and derivatives is calibrated.  ``y`` as for ``point_log_prob``."""
        return self._point_density(y)[0]

    def rsample(self, sample_shape=torch.Size(), base_samples=None):
        """mean + chol(Sigma) eps: exact Cholesky root on the GPU (fp64 blocked MFMA factorisation) where gpytorch switches
        to a Lanczos root above ``max_cholesky_size``.  Shape ``sample_shape + [B(p+1)]``."""
        self._ensure_joint()
        eng = self.model.engine
        if self._root is None:
            self._root = eng.covariance_root(self._Sigma)
        n_out = self._mu.shape[0]
        sample_shape = torch.Size(sample_shape)
        n = int(sample_shape.numel()) if len(sample_shape) else 1
        if base_samples is None:
            eps = torch.randn(n, n_out, dtype=self._mu.dtype, device=self._mu.device)
        else:
            eps = base_samples.reshape(n, n_out).to(self._mu.dtype)
        return eng.draw(self._mu, self._root, eps).reshape(tuple(sample_shape) + (n_out,))

    def sample(self, sample_shape=torch.Size(), base_samples=None):
        with torch.no_grad():
            return self.rsample(sample_shape, base_samples)


class _ApproximateMLL(torch.nn.Module):
    mll_type = "ELBO"

    def __init__(self, likelihood, model, num_data, beta=1.0):
        super().__init__()
        if beta != 1.0:
            raise NotImplementedError("beta != 1 is not used by the reference harness")
        self.likelihood, self.model, self.num_data = likelihood, model, num_data

    def forward(self, output, target):
        if not isinstance(output, PredictiveDistribution) or output.likelihood is None:
            raise TypeError("mll expects likelihood(model(x, derivative_directions=D)) as in directional_vi.py:245")
        model = output.model
        plist = model._param_list(self.likelihood)
        dp = getattr(model, "data_parallel", None)
        elbo, mu, varn = _ElboFunction.apply(model.engine, output.x, target, output.D, float(self.num_data),
                                             self.mll_type, dp, _param_names(model, self.likelihood), *plist)
        # the ELBO fast path does not form per-output variances; they are produced on demand
        output._mu, output._varn = mu, (varn if varn.numel() else None)
        return elbo


    @torch.no_grad()
    def backward_step(self, output, target):
        """``loss = -mll(output, target); loss.backward()`` of the reference loop (directional_vi.py:245-247) without the
        autograd round trip: the engine's gradient buffers become the parameters' ``.grad`` directly (the chain
        loss -> mll multiplies them by (-1)(-1) = 1, so the numbers are the same; six tiny elementwise launches and one pass
        over the 36 MB L_S gradient fewer per step).  Returns the loss as a device scalar."""
        if not isinstance(output, PredictiveDistribution) or output.likelihood is None:
            raise TypeError("mll expects likelihood(model(x, derivative_directions=D)) as in directional_vi.py:245")
        model = output.model
        plist = model._param_list(self.likelihood)
        names = _param_names(model, self.likelihood)
        pd = dict(zip(names, [_ops.detach_keep(p) for p in plist]))
        dp = getattr(model, "data_parallel", None)
        if dp is not None:
            loss, grads, mu, varn = dp.loss_and_grads(model.engine, pd, output.x, target, output.D, float(self.num_data),
                                                      self.mll_type)
        else:
            loss, grads, mu, varn = model.engine.loss_and_grads(pd, output.x, target, output.D, float(self.num_data),
                                                                self.mll_type)
        for p, k in zip(plist, names):
            if isinstance(p, torch.nn.Parameter) and p.requires_grad:
                g = grads[k].view_as(p)
                p.grad = g if p.grad is None else p.grad.add_(g)
        output._mu, output._varn = mu, (varn if varn.numel() else None)
        return loss


class VariationalELBO(_ApproximateMLL):
    mll_type = "ELBO"


class PredictiveLogLikelihood(_ApproximateMLL):
    mll_type = "PLL"


class ApproximateGP(torch.nn.Module):
    def __init__(self, variational_strategy):
        super().__init__()
        self.variational_strategy = variational_strategy
        self._engine = None
        # None: ``self(x, derivative_directions=D)`` takes the model's own number of directions per data point (the reference's
        # assertion).  int pd: the call takes exactly pd per point (``None`` / empty for 0) and the ``mll(...)`` / ``backward_step``
        # route trains on them (ElboEngine.loss_and_grads with pd != p: float32, Cholesky whitening, one rank)
        self.data_directions = None

    @property
    def engine(self):
        Z = self.variational_strategy.inducing_points
        cls = ElboEngine
        if Z.dtype == torch.float64:        # model built under torch.set_default_dtype(torch.float64) (exp_script.py:56)
            from ._step64 import ElboEngine64 as cls
        if self._engine is None or self._engine.device != Z.device or type(self._engine) is not cls:
            self._engine = cls(Z.device)
        return self._engine

    def variational_parameters(self):
        for mod in self.modules():
            if isinstance(mod, _VariationalDistribution):
                for p in mod.parameters(recurse=False):
                    yield p

    def hyperparameters(self):
        for mod in self.modules():
            if not isinstance(mod, _VariationalDistribution):
                for p in mod.parameters(recurse=False):
                    yield p

    def fit_variational(self, likelihood, dataset_or_tensors, minibatch_size=4096, data_directions=None, num_data=None, seed=None):
        """q(u) <- its closed-form optimum for the current hyper-parameters and inducing set, from one pass over the data: the method
        form of ``directional_vi.fit_variational`` (Titsias 2009; ``ElboEngine.collapsed_accumulator``).  Returns the result object."""
        from .directional_vi import fit_variational
        return fit_variational(self, likelihood, dataset_or_tensors, minibatch_size=minibatch_size, data_directions=data_directions,
                               num_data=num_data, seed=seed)

    def collapsed_loss_and_grads(self, likelihood, dataset_or_tensors, minibatch_size=4096, data_directions=None, num_data=None, seed=None,
                                 workspace_budget=1 << 30, write_variational=True):
        """The collapsed bound (the ELBO with q(u) at its closed-form optimum) from two passes over the data, its gradients written to
        ``.grad`` of the hyper-parameters, inducing points and directions: the method form of
        ``directional_vi.collapsed_loss_and_grads`` (``CollapsedAccumulator.add_backward``).  Returns the result object."""
        from .directional_vi import collapsed_loss_and_grads
        return collapsed_loss_and_grads(self, likelihood, dataset_or_tensors, minibatch_size=minibatch_size, data_directions=data_directions,
                                        num_data=num_data, seed=seed, workspace_budget=workspace_budget,
                                        write_variational=write_variational)

    # ---- posterior mean without the predictive distribution (what the reference's mean-only callers read from
    #      ``likelihood(model(x, derivative_directions=D)).mean``: experiments/bunny/exp_bunny.py:189-195,
    #      experiments/rover/bo_traditional.py:214, experiments/GNN_bo/bo.py:172) ----
    def _mean_predictor(self):
        """The engine's ``MeanPredictor`` for the current parameters.  Eval mode: cached on the model, keyed by
        (data_ptr, _version) of the parameters like the engine's evaluation cache -- an optimizer step or ``load_state_dict``
        changes the key; training mode: rebuilt per call."""
        engine = self.engine            # (ElboEngine64 -- a float64 model -- refuses: NotImplementedError)
        vs = self.variational_strategy
        if hasattr(vs, "_strategy_is_updated") and not vs._strategy_is_updated():
            vs._whiten_legacy_parameters()
        if self.training and hasattr(vs, "_maybe_init"):
            vs._maybe_init()
        params = self._param_dict(None)
        # (the mean does not depend on the likelihood noise, whose stand-in is a fresh tensor per call)
        key = tuple((t.data_ptr(), t._version) for k, t in params.items() if k != "raw_noise")
        key += (engine.whitening, engine.data_outputs, engine.shared_directions)
        cached = self.__dict__.get("_mean_cache")
        if not self.training and cached is not None and cached[0] == key and cached[1] is engine:
            return cached[2]
        pred = engine.mean_predictor(params)
        self.__dict__["_mean_cache"] = (key, engine, pred) if not self.training else None
        return pred

    def sample_paths(self, num_samples, num_features=2048, generator=None, base_samples=None):
        """``num_samples`` draws of the posterior FUNCTION f for the current parameters (``ElboEngine.sample_paths``): a
        ``SamplePaths`` whose ``values(x)`` [n, B], ``values_and_gradients(x)`` and ``paths(x, derivative_directions)`` evaluate the
        SAME functions at any number of points in any number of batches -- what a Thompson sampler takes from
        ``preds.sample(torch.Size([n]))`` without anything of size B' x B'.  Paths are of f: a likelihood's white noise is the
        caller's to add.  An explicit object: nothing is cached on the model.  Not differentiable."""
        engine = self.engine            # (ElboEngine64 -- a float64 model -- refuses: NotImplementedError)
        vs = self.variational_strategy
        if hasattr(vs, "_strategy_is_updated") and not vs._strategy_is_updated():
            vs._whiten_legacy_parameters()
        if self.training and hasattr(vs, "_maybe_init"):
            vs._maybe_init()
        return engine.sample_paths(self._param_dict(None), num_samples, num_features, generator, base_samples)

    def thompson_step(self, candidates, lower, upper, num_samples, num_starts=8, iterations=20, num_features=2048, maximize=False,
                      generator=None):
        """``sample_paths(num_samples, num_features, generator)`` followed by ``directional_vi.thompson_candidates``: per draw the
        best of ``num_starts`` candidates refined on that draw inside the box -> (x_next [n, d], f_next [n], f_candidates_best [n]).
        Refuses where ``sample_paths`` refuses (CIQ whitening, float64 models)."""
        from .directional_vi import thompson_candidates
        paths = self.sample_paths(num_samples, num_features, generator)
        return thompson_candidates(paths, candidates, lower, upper, num_starts, iterations, maximize)

    # ---- posterior variance with its gradient and the acquisitions on it (what the reference's confidence-bound callers read from
    #      ``preds.variance``: experiments/rover/bo_traditional.py:214, experiments/GNN_bo/bo.py:171-173) ----
    def _variance_predictor(self):
        """The engine's ``VariancePredictor`` for the current parameters, cached in eval mode and keyed like ``_mean_predictor``"""
        engine = self.engine            # (ElboEngine64 -- a float64 model -- refuses: NotImplementedError)
        vs = self.variational_strategy
        if hasattr(vs, "_strategy_is_updated") and not vs._strategy_is_updated():
            vs._whiten_legacy_parameters()
        if self.training and hasattr(vs, "_maybe_init"):
            vs._maybe_init()
        params = self._param_dict(None)
        key = tuple((t.data_ptr(), t._version) for k, t in params.items() if k != "raw_noise")
        key += (engine.whitening, engine.data_outputs, engine.shared_directions)
        cached = self.__dict__.get("_variance_cache")
        if not self.training and cached is not None and cached[0] == key and cached[1] is engine:
            return cached[2]
        pred = engine.variance_predictor(params)
        self.__dict__["_variance_cache"] = (key, engine, pred) if not self.training else None
        return pred

    def posterior_variance(self, x, likelihood=None):
        """Variance [B] of the function value at x [B, d] under q(f) (``likelihood`` given: plus its noise), from
        ``ElboEngine.variance_predictor``: one fp64 product per batch, no solve.  Not differentiable."""
        var = self._variance_predictor().variance(x)
        return var if likelihood is None else (var + likelihood.noise.detach().reshape(()).to(var)).clamp_min_(1e-6)

    def posterior_variance_gradient(self, x):
        """Gradient [B, d] of the variance of the function value at x [B, d]"""
        return self._variance_predictor().variance_and_gradient(x)[1]

    def acquisition(self, x, kind="lcb", beta=2.0, best=None, maximize=False):
        """Acquisition values [B] at x [B, d], smaller is better: "lcb_var" mu - beta sigma^2, "lcb" mu - beta sigma, "ei" the
        negative expected improvement below ``best`` (``VariancePredictor.acquisition``)"""
        return self._variance_predictor().acquisition(x, kind, beta, best, maximize)

    def acquisition_step(self, candidates, lower, upper, kind="lcb", beta=2.0, best=None, maximize=False, num_starts=8, iterations=20):
        """``directional_vi.acquisition_candidates`` on this model's ``VariancePredictor``: the acquisition over the candidates, its
        ``num_starts`` best refined by the on-device descent inside the box -> (x_next [d], a_next, a_candidates_best).  Refuses where
        ``variance_predictor`` refuses (ARD, Matern-5/2, CIQ whitening, float64 models)."""
        from .directional_vi import acquisition_candidates
        return acquisition_candidates(self._variance_predictor(), candidates, lower, upper, kind, beta, best, maximize, num_starts,
                                      iterations)

    def posterior_mean(self, x, derivative_directions=None):
        """Predictive mean at x [B, d]: [B (pd + 1)] interleaved with pd = len(derivative_directions) // B rows per point
        (``None``: function values only); equals ``likelihood(self(x, derivative_directions=D)).mean`` without assembling
        K_ZX or solving against K_ZZ per batch (``ElboEngine.mean_predictor``).  Not differentiable."""
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        return self._mean_predictor().mean(x, derivative_directions)

    def posterior_mean_gradient(self, x):
        """Gradient of the predictive mean of f at x [B, d] -> [B, d] (all d partial derivatives, whatever the number of
        directions the model was trained with)"""
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        return self._mean_predictor().value_and_gradient(x)[1]

    def posterior_mean_hvp(self, x, v):
        """Hessian of the predictive mean of f times one vector per point: grad^2 mu_f(x_b) v_b, x and v [B, d] -> [B, d]
        (``MeanPredictor.hvp``; v is used as given)"""
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        return self._mean_predictor().hvp(x, v)

    def posterior_mean_hessian(self, x):
        """Hessian of the predictive mean of f at x [B, d] -> [B, d, d], symmetric (``MeanPredictor.hessian``: d products)"""
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        return self._mean_predictor().hessian(x)

    def posterior_gradient(self, x, likelihood=None):
        """The distribution of (f(x), grad f(x)) at every point of x [B, d], whatever number of directions the model was trained
        with: a named tuple of value_mean [B], value_variance [B], gradient_mean [B, d], gradient_covariance [B, d, d] and
        value_gradient_covariance [B, d] (``likelihood`` given: with its noise on the variances).  ``posterior`` with ``eye(d)``
        tiled over the points and its ``point_covariances``: u^T gradient_covariance u is the variance of the derivative along
        u.  d <= 95 (float32 Cholesky-whitened models; CIQ whitening at d == p gives diagonal blocks)."""
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        B, d = x.shape
        if d > 95:
            raise ValueError("posterior_gradient takes all d partial derivatives as data directions: at most 95, got d = %d" % d)
        post = self.posterior(x, torch.eye(d, dtype=x.dtype, device=x.device).repeat(B, 1), likelihood)
        blocks = post.point_covariances
        mu = post.mean.reshape(B, d + 1)
        return PosteriorGradient(mu[:, 0], blocks[:, 0, 0], mu[:, 1:], blocks[:, 1:, 1:], blocks[:, 1:, 0])

    def _gradient_posterior(self, x, likelihood, what):
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        B, d = x.shape
        if d > 95:
            raise ValueError("%s takes all d partial derivatives as data directions: at most 95, got d = %d" % (what, d))
        return self.posterior(x, torch.eye(d, dtype=x.dtype, device=x.device).repeat(B, 1), likelihood), B, d

    def sample_gradients(self, x, num_samples, likelihood=None, base_samples=None):
        """``num_samples`` draws of (f(x), grad f(x)) at every point of x [B, d]: (values [n, B], gradients [n, B, d]), exact
        within a point (value and all d partial derivatives jointly) and independent between points
        (``posterior(...).sample_points``; ``sample`` is the jointly correlated form).  q(f) without a ``likelihood``, with its
        noise otherwise; ``base_samples``: n B (d + 1) standard normal numbers instead of ``torch.randn``.  Whatever number of
        directions the model was trained with, through ``posterior_gradient``'s tiled ``eye(d)``; d <= 95."""
        post, B, d = self._gradient_posterior(x, likelihood, "sample_gradients")
        draws = post.sample_points(torch.Size([int(num_samples)]), base_samples).reshape(int(num_samples), B, d + 1)
        return draws[:, :, 0], draws[:, :, 1:]

    def gradient_log_prob(self, x, y, likelihood):
        """[B]: the joint log-density of y[b] = (value, d partial derivatives) [B, d + 1] under the model's predictive
        distribution of (f(x_b), grad f(x_b)) with the likelihood's noise, point by point (``posterior(...).point_log_prob``).
        Whatever number of directions the model was trained with; d <= 95."""
        post, B, d = self._gradient_posterior(x, likelihood, "gradient_log_prob")
        if tuple(y.shape) != (B, d + 1):
            raise ValueError("y must be [B, d + 1] = [%d, %d], got %s" % (B, d + 1, tuple(y.shape)))
        return post.point_log_prob(y)

    def posterior(self, x, derivative_directions=None, likelihood=None):
        """Predictive distribution at x [B, d] over B (pd + 1) interleaved outputs, pd = len(derivative_directions) // B ANY
        number of directions per point up to 95 (``None``: the B function values; ``eye(d)`` tiled: values and full gradients),
        whatever number p the model was trained with.  ``likelihood`` given: with its noise, as ``likelihood(self(x, ...))``;
        else q(f), as ``self(x, ...)``.  With pd == p it IS that distribution (``self(x, derivative_directions=D)`` keeps the
        reference's assertion on a count mismatch); otherwise K_ZX comes from the rectangular assembly
        (``ElboEngine.predict``: float32 Cholesky-whitened models).  ``mean``, ``variance``, ``stddev``, ``confidence_region``,
        ``covariance_matrix``, ``rsample`` and ``sample`` work; ``value_variance`` is ``variance[::pd + 1]``."""
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        vs = self.variational_strategy
        if hasattr(vs, "_strategy_is_updated") and not vs._strategy_is_updated():
            vs._whiten_legacy_parameters()
        if self.training and hasattr(vs, "_maybe_init"):
            vs._maybe_init()
        D = derivative_directions
        if D is not None:
            D = D.to(x.device)
            if D.numel() and (D.dim() != 2 or x.shape[0] == 0 or D.shape[0] % x.shape[0] or D.shape[1] != x.shape[1]):
                raise ValueError("derivative_directions must be [B * pd, d] = [%d * pd, %d], got %s"
                                 % (x.shape[0], x.shape[1], tuple(D.shape)))
        out = PredictiveDistribution(self, x, D, likelihood)
        pd = D.shape[0] // x.shape[0] if D is not None and D.numel() else 0
        out._value_stride = 1 if getattr(vs, "data_outputs", "all") == "values" else pd + 1     # (derivative-free data: B outputs)
        return out

    def __call__(self, inputs, prior=False, **kwargs):
        if inputs.dim() == 1:
            inputs = inputs.unsqueeze(-1)
        return self.variational_strategy(inputs, prior=prior, **kwargs)
