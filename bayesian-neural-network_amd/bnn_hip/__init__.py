"""bnn_hip — host side of the MI355X Bayes-by-backprop hot path.

`_lib`       ctypes binding of libbnn_hip.so (include/bnn_hip.h); raises if it is missing
`ops`        one function per C-ABI entry point, on torch device tensors
`functional` autograd bridges (forward = HIP kernels)
`engine`     batched-samples launcher + MC-sample sharding over torch.distributed
`runtime`    process-wide knobs: math mode, Philox seed / sample counter, sharding switch
`optim`      FusedAdam / FusedSGD: torch.optim.Adam's / SGD's update in one launch (F2, K6)
`train`      GraphedTrainStep: zero_grad -> sample_elbo -> backward -> Adam as one hipGraph
`dense_train` GraphedDenseTrainStep: the same for MLP / MLP_Dropout (forward, loss, backward, SGD / Adam) (K6)
`capture`    what every captured object shares: the optimiser's sample counter, warm-up and its undo, side-stream capture
`synth`      synthetic inputs with the reference's distributions (numpy only)
`active`     ActivePool / ActiveLearner: pool scoring, top-k acquisition and training on the labelled subset (F10); BatchBALD batches
             chosen jointly (joint_probs / acquire_batchbald, F15)
`flipout`    FlipoutLinear / FlipoutNetwork: the Flipout estimator on BayesianLinear's parameters, per-row weight noise (F16)
`laplace`    DiagLaplace: a diagonal Laplace posterior for a trained MLP / MLP_Dropout, Fisher accumulation on the device, the prior
             precision by the marginal likelihood, the result a BayesianNetwork (F17)
`diagnostics` PosteriorStats: weight / sigma / SNR / posterior-sample histograms of a model in one device pass (F11)
`sgmcmc`     FusedSGMCMC / WeightBank: SGLD / SGHMC in the optimiser's place of K6's captured step, the samples filed into a
             device-resident bank of weight sets that predicts as an ensemble, one launch per layer for all members (F19)
`kfac`       KronLaplace: the Kronecker-factored (KFAC) Laplace posterior -- factor accumulation, evidence, GLM predictive and
             matrix-normal weight draws into a WeightBank, in the Kronecker eigenbasis (F20)
`ensemble`   DeepEnsemble / EnsembleTrainStep: a deep ensemble trained in place in a WeightBank, every member per launch, one
             captured training step whatever the number of members (F21)
`swag`       FusedSWAG / SwagPosterior: SGD with momentum in the optimiser's place of K6's captured step that also collects SWAG's
             moments, the SWA point estimate, SWAG-Diagonal as a BayesianNetwork and low-rank draws into a WeightBank (F22)
`svgd`       SteinTransform: SVGD / kde-WGD repulsive ensembles -- the members of a DeepEnsemble coupled through an RBF kernel, the
             gradient bucket rewritten into the Stein direction by three launches inside EnsembleTrainStep (F23)
`ivon`       FusedIVON: the variational online Newton optimiser in K6's captured step -- a weight draw in front of each forward
             pass, one natural-gradient launch behind the backward pass; the posterior as a BayesianNetwork and as draws into a
             WeightBank (F24)
"""
from .runtime import get_math, manual_seed, set_host_eps, set_math, shard_samples  # noqa: F401
from ._lib import BnnHipError  # noqa: F401
from .active import ActiveLearner, ActivePool  # noqa: F401
from .laplace import DiagLaplace  # noqa: F401
from .sgmcmc import FusedSGMCMC, WeightBank  # noqa: F401
from .swag import FusedSWAG, SwagPosterior  # noqa: F401
from .kfac import KronLaplace  # noqa: F401
from .ensemble import DeepEnsemble, EnsembleTrainStep  # noqa: F401
from .svgd import SteinTransform  # noqa: F401
from .ivon import FusedIVON  # noqa: F401

__all__ = ["get_math", "set_math", "manual_seed", "set_host_eps", "shard_samples", "BnnHipError", "ActiveLearner", "ActivePool", "DiagLaplace",
           "FusedSGMCMC", "WeightBank", "KronLaplace", "DeepEnsemble", "EnsembleTrainStep",
           "FusedSWAG", "SwagPosterior", "SteinTransform", "FusedIVON"]
