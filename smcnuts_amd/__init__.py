"""smcnuts_amd: the SMC-NUTS hot path on MI355X (gfx950).

Host side mirrors the reference's operator interface
(UoL-SignalProcessingGroup/SMC-NUTS: SMCSampler, Samples, NUTSProposal,
ForwardLKernel, GaussianApproxLKernel, ESSTempering, Estimate, StanModel-shaped
targets); the compute is hand-written HIP behind the C ABI of
include/smcnuts_hip.h (libsmcnuts_hip.so), reached through ctypes.  No PyTorch
on this path and no CPU fallback.
"""
from .smc_sampler import SMCSampler  # noqa: F401
from .model.targets import (ArmaModel, CategoricalRegression, ContinuousGLM, GammaRegression, GaussianTarget,  # noqa: F401
                            GLMTarget, HierarchicalGLM, HostTarget, IsoGaussian, LinearRegression, LogisticRegression,
                            MultilevelGLM, NegativeBinomialRegression, OrdinalRegression, PoissonRegression, PRMwCDModel,
                            RobustRegression, StanModel, WideGLMTarget)
from .calibration import Calibration, combine_calibration_partials  # noqa: F401
from .criteria import Pointwise, combine_pointwise_partials, compare  # noqa: F401
from .psis import PsisLoo, compare_loo, merge_candidates, tail_len  # noqa: F401
from .predict import Prediction, PredictiveDraws, combine_predict_partials, compare_heldout  # noqa: F401
from .forecast import Forecast, combine_forecast_partials  # noqa: F401
from .residuals import OneStepResiduals, combine_residual_partials  # noqa: F401
from .summary import PosteriorSummary  # noqa: F401
from .covariance import PosteriorCovariance, combine_cov_partials, device_covariance  # noqa: F401
from .stepsize import StepSizeProbe, choose_step_size, combine_stepsize_partials  # noqa: F401
