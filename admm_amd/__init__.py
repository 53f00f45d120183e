"""admm_amd -- MI355X (gfx950) ADMM solvers behind the R interface of yixuan/ADMM.

Only what the hot path needs: `csrc/` (HIP kernels + the C ABI of include/admm_hip.h, built into
lib/libadmm_hip.so by `python -m admm_amd.build`) and `api.py`, the host-side mirror of the
reference's `admm_lasso()/admm_enet()/admm_lad()/admm_bp()` builder chain.
"""
from .api import (LassoPlan, ADMM_BP, ADMM_Dantzig, ADMM_Enet, ADMM_GrpLasso, ADMM_LAD, ADMM_Lasso, admm_bp, admm_dantzig, admm_enet,
                  admm_grplasso, admm_lad, admm_lasso, admm_quantreg, ADMM_QuantReg, admm_huber, ADMM_Huber, admm_logit, ADMM_Logit, admm_logit_multi, ADMM_LogitMulti, admm_logit_ovr, ADMM_LogitOvR, admm_logit_ridge, ADMM_LogitRidge, admm_logit_ridge_ovr, ADMM_LogitRidgeOvR, admm_logit_enet, ADMM_LogitEnet, admm_logit_enet_ovr, ADMM_LogitEnetOvR, admm_poisson, ADMM_Poisson, admm_logit_enet_cv, ADMM_LogitEnetCV, admm_poisson_cv, ADMM_PoissonCV, admm_mtlasso, ADMM_MTLasso, admm_sgl, ADMM_SGL, admm_boxenet, ADMM_BoxEnet)
from ._lib import AdmmHipError, DevicePtr, last_parallel_layout, load, options

__all__ = ["admm_lasso", "admm_enet", "admm_grplasso", "ADMM_GrpLasso", "admm_sgl", "ADMM_SGL", "admm_boxenet", "ADMM_BoxEnet", "admm_mtlasso", "ADMM_MTLasso", "admm_lad", "admm_quantreg", "ADMM_QuantReg", "admm_huber", "ADMM_Huber", "admm_logit", "ADMM_Logit", "admm_logit_multi", "ADMM_LogitMulti", "admm_logit_ovr", "ADMM_LogitOvR", "admm_logit_ridge", "ADMM_LogitRidge", "admm_logit_ridge_ovr", "ADMM_LogitRidgeOvR", "admm_logit_enet", "ADMM_LogitEnet", "admm_logit_enet_ovr", "ADMM_LogitEnetOvR", "admm_poisson", "ADMM_Poisson", "admm_logit_enet_cv", "ADMM_LogitEnetCV", "admm_poisson_cv", "ADMM_PoissonCV", "admm_bp", "admm_dantzig", "ADMM_Dantzig", "ADMM_Lasso", "ADMM_Enet", "ADMM_LAD", "ADMM_BP",
           "LassoPlan", "DevicePtr", "AdmmHipError", "load", "options", "last_parallel_layout"]
