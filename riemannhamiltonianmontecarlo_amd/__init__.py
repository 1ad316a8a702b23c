"""MI355X-native RMHMC hot path (Bayesian logistic regression).

Host side of the C-ABI in include/rmhmc.h; mirrors the reference's
``code/rmhmc.py`` interface.  See DESIGN.md.
"""
from .rmhmc import RMHMC  # noqa: F401
from .hmc import HMC  # noqa: F401
from .mmala import mMALA  # noqa: F401
from .metropolis import AMH  # noqa: F401
from .iwls import iwls  # noqa: F401
from .gibbs_sampler import auxiliary_gibbs  # noqa: F401
from .phmc import PHMC  # noqa: F401
from .evidence import log_evidence, log_evidence_adaptive  # noqa: F401
from .predict import posterior_predictive  # noqa: F401
from .loo import psis_loo  # noqa: F401
from . import tools, data, experiment, evidence, predict, loo  # noqa: F401

__all__ = ["RMHMC", "HMC", "mMALA", "AMH", "iwls", "auxiliary_gibbs", "PHMC", "log_evidence", "log_evidence_adaptive", "posterior_predictive", "psis_loo",
           "tools", "data", "experiment", "evidence", "predict", "loo"]
