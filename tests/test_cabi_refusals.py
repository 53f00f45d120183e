"""What the C ABI refuses, pinned without a GPU: one bad call per rule and entry point, with the exact return code and
admm_hip_last_error() text.  Every argument check of the library runs before it looks for a device, so all of this is observable
on a machine without one.  The expected strings in TABLE are literals recorded from the library as it was before the entry points
were rebuilt on call_args.h (the rows that were allowed to change are marked); they are not read from the code under test."""
import ctypes
import os

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE = 1, 2

_PATH = "lambda_in nlambda_in nlambda_auto lmin_ratio standardize intercept"
_OUT = "lambda_out beta_out niter_out stats"
_TRACE = "trace_out trace_cap ntrace_out"
_STATE = "state_out state_cap nstate_out"
_DENSE_OUT = "opts dbeta_out niter_out stats"
# the parameters of every entry point, by the names the rules below override (include/admm_hip.h has the declarations)
SIGNATURES = {
    "lasso": f"x y n p mem {_PATH} opts {_OUT}",
    "enet": f"x y n p mem {_PATH} alpha opts {_OUT}",
    "lasso_cv": f"x y n p mem fold_id nfolds {_PATH} alpha opts lambda_out beta_out niter_out cv_mean cv_se fold_mse fold_niter fold_beta idx_min idx_1se stats",
    "lasso_multi": f"x y n p m mem {_PATH} alpha opts {_OUT}",
    "parlasso": f"x y n p mem {_PATH} nthread opts {_OUT}",
    "lad": f"x y n p mem intercept {_DENSE_OUT}",
    "lad_traced": f"x y n p mem intercept {_DENSE_OUT} {_TRACE}",
    "lad_state": f"x y n p mem intercept {_DENSE_OUT} {_TRACE} {_STATE}",
    "bp": f"x y n p mem {_DENSE_OUT}",
    "bp_traced": f"x y n p mem {_DENSE_OUT} {_TRACE}",
    "bp_state": f"x y n p mem {_DENSE_OUT} {_TRACE} {_STATE}",
    "dantzig": f"x y n p mem {_PATH} opts lambda_out dbeta_out niter_out stats",
    "dantzig_traced": f"x y n p mem {_PATH} opts lambda_out dbeta_out niter_out stats {_TRACE}",
    "parbp": f"x y n p mem nthread {_DENSE_OUT}",
    "parbp_traced": f"x y n p mem nthread {_DENSE_OUT} {_TRACE}",
    "parbp_dist": f"x y n p p_total col_offset mem nthread {_DENSE_OUT}",
    "lasso_plan_create": f"x y n p mem {_PATH} alpha nthread opts plan_out nlambda_out",
    "lasso_plan_create_dist": f"x y n n_total p mem {_PATH} nthread opts plan_out nlambda_out",
    "lasso_plan_create_dist_cols": f"x y n p p_total col_offset mem {_PATH} alpha opts plan_out nlambda_out",
    "lasso_dist": f"x y n n_total p mem {_PATH} alpha opts {_OUT}",
    "parlasso_dist": f"x y n n_total p mem {_PATH} nthread opts {_OUT}",
    "lasso_dist_cols": f"x y n p p_total col_offset mem {_PATH} alpha opts {_OUT}",
}
# the 8 doubles of x are read as 4 x 2 by default; BP, ParBP and Dantzig need more columns than that and read them as 2 x 4
SHAPES = {e: (2, 4) for e in ("bp", "bp_traced", "bp_state", "dantzig", "dantzig_traced", "parbp", "parbp_traced", "parbp_dist")}
DIST = ("parbp_dist", "lasso_plan_create_dist", "lasso_plan_create_dist_cols", "lasso_dist", "parlasso_dist", "lasso_dist_cols")

# rule -> the arguments it spoils.  opts: (maxit, eps_abs, eps_rel, rho); lambda_in: the grid's values
RULES = {
    "null_x": dict(x=None),
    "n_zero": dict(n=0),
    "bad_mem": dict(mem=7),
    "null_opts": dict(opts=None),
    "maxit_zero": dict(opts=(0, 1e-5, 1e-5, 1.0)),
    "neg_eps": dict(opts=(10, -1.0, 1e-5, 1.0)),
    "nlambda_neg": dict(nlambda_in=-1),
    "no_grid": dict(nlambda_in=0, nlambda_auto=0),
    "lmin_one": dict(lmin_ratio=1.0),
    "neg_lambda": dict(lambda_in=(0.5, -1.0), nlambda_in=2),
    "alpha_big": dict(alpha=1.5),
    "alpha_neg": dict(alpha=-0.5),
    "null_out": dict(lambda_out=None, dbeta_out=None, plan_out=None),
    "trace_null": dict(trace_cap=4, trace_out=None),
    "state_no_trace": dict(state_cap=4, trace_cap=0),
    "rho_zero": dict(opts=(10, 1e-5, 1e-5, 0.0)),
    "lad_wide": dict(n=2, p=4),
    "bp_tall": dict(n=4, p=2),
    "dantzig_p2": dict(n=4, p=2),
    "nthread_zero": dict(nthread=0),
    "nthread_big": dict(nthread=5),
    "nfolds_one": dict(nfolds=1),
    "fold_id_bad": dict(fold_id=(0, 1, 0, 2), nfolds=2),
    "m_zero": dict(m=0),
    "col_block": dict(col_offset=7),
    "n_total_small": dict(n_total=2),
    "no_comm": dict(),
    "maxit_zero+nlambda_neg": dict(opts=(0, 1e-5, 1e-5, 1.0), nlambda_in=-1),
}
_GRID = [e for e, s in SIGNATURES.items() if "nlambda_in" in s]
_ALL = list(SIGNATURES)
# rule -> the entry points it concerns
CONCERNS = {
    **{r: _ALL for r in ("null_x", "n_zero", "bad_mem", "null_opts", "maxit_zero", "neg_eps", "null_out")},
    **{r: _GRID for r in ("nlambda_neg", "no_grid", "lmin_one", "neg_lambda", "maxit_zero+nlambda_neg")},
    "alpha_big": [e for e, s in SIGNATURES.items() if "alpha" in s.split()],
    "alpha_neg": ["enet"],
    "trace_null": [e for e, s in SIGNATURES.items() if "trace_cap" in s],
    "state_no_trace": ["lad_state", "bp_state"],
    "rho_zero": [e for e, s in SIGNATURES.items() if "dbeta_out" in s and "lambda_out" not in s],
    "lad_wide": ["lad", "lad_traced", "lad_state"],
    "bp_tall": ["bp", "bp_traced", "bp_state", "parbp", "parbp_traced"],
    "dantzig_p2": ["dantzig", "dantzig_traced"],
    "nthread_zero": ["parlasso", "parbp", "parbp_traced", "parbp_dist"],
    "nthread_big": ["parlasso", "parbp", "parbp_traced", "parbp_dist", "lasso_plan_create"],
    "nfolds_one": ["lasso_cv"],
    "fold_id_bad": ["lasso_cv"],
    "m_zero": ["lasso_multi"],
    "col_block": ["parbp_dist", "lasso_plan_create_dist_cols", "lasso_dist_cols"],
    "n_total_small": ["lasso_plan_create_dist", "lasso_dist", "parlasso_dist"],
    "no_comm": list(DIST),
}

# (entry point, rule, return code, admm_hip_last_error())
TABLE = [
    ('lasso', 'null_x', 1, 'x and y must not be NULL'),
    ('enet', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso_cv', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso_multi', 'null_x', 1, 'x and y must not be NULL'),
    ('parlasso', 'null_x', 1, 'x and y must not be NULL'),
    ('lad', 'null_x', 1, 'x and y must not be NULL'),
    ('lad_traced', 'null_x', 1, 'x and y must not be NULL'),
    ('lad_state', 'null_x', 1, 'x and y must not be NULL'),
    ('bp', 'null_x', 1, 'x and y must not be NULL'),
    ('bp_traced', 'null_x', 1, 'x and y must not be NULL'),
    ('bp_state', 'null_x', 1, 'x and y must not be NULL'),
    ('dantzig', 'null_x', 1, 'x and y must not be NULL'),
    ('dantzig_traced', 'null_x', 1, 'x and y must not be NULL'),
    ('parbp', 'null_x', 1, 'x and y must not be NULL'),
    ('parbp_traced', 'null_x', 1, 'x and y must not be NULL'),
    ('parbp_dist', 'null_x', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso_plan_create_dist', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso_plan_create_dist_cols', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso_dist', 'null_x', 1, 'x and y must not be NULL'),
    ('parlasso_dist', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso_dist_cols', 'null_x', 1, 'x and y must not be NULL'),
    ('lasso', 'n_zero', 1, 'n and p must be positive'),
    ('enet', 'n_zero', 1, 'n and p must be positive'),
    ('lasso_cv', 'n_zero', 1, 'n and p must be positive'),
    ('lasso_multi', 'n_zero', 1, 'n and p must be positive'),
    ('parlasso', 'n_zero', 1, 'n and p must be positive'),
    ('lad', 'n_zero', 1, 'n and p must be positive'),
    ('lad_traced', 'n_zero', 1, 'n and p must be positive'),
    ('lad_state', 'n_zero', 1, 'n and p must be positive'),
    ('bp', 'n_zero', 1, 'n and p must be positive'),
    ('bp_traced', 'n_zero', 1, 'n and p must be positive'),
    ('bp_state', 'n_zero', 1, 'n and p must be positive'),
    ('dantzig', 'n_zero', 1, 'n and p must be positive'),
    ('dantzig_traced', 'n_zero', 1, 'n and p must be positive'),
    ('parbp', 'n_zero', 1, 'n and p must be positive'),
    ('parbp_traced', 'n_zero', 1, 'n and p must be positive'),
    ('parbp_dist', 'n_zero', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'n_zero', 1, 'n and p must be positive'),
    ('lasso_plan_create_dist', 'n_zero', 1, 'n_total must be >= n_local > 0'),
    ('lasso_plan_create_dist_cols', 'n_zero', 1, 'n and p must be positive'),
    ('lasso_dist', 'n_zero', 1, 'n_total must be >= n_local > 0'),
    ('parlasso_dist', 'n_zero', 1, 'n_total must be >= n_local > 0'),
    ('lasso_dist_cols', 'n_zero', 1, 'n and p must be positive'),
    ('lasso', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('enet', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso_cv', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso_multi', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('parlasso', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lad', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lad_traced', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lad_state', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('bp', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('bp_traced', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('bp_state', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('dantzig', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('dantzig_traced', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('parbp', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('parbp_traced', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('parbp_dist', 'bad_mem', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso_plan_create_dist', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso_plan_create_dist_cols', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso_dist', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('parlasso_dist', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso_dist_cols', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('lasso', 'null_opts', 1, 'opts must not be NULL'),
    ('enet', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso_cv', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso_multi', 'null_opts', 1, 'opts must not be NULL'),
    ('parlasso', 'null_opts', 1, 'opts must not be NULL'),
    ('lad', 'null_opts', 1, 'opts must not be NULL'),
    ('lad_traced', 'null_opts', 1, 'opts must not be NULL'),
    ('lad_state', 'null_opts', 1, 'opts must not be NULL'),
    ('bp', 'null_opts', 1, 'opts must not be NULL'),
    ('bp_traced', 'null_opts', 1, 'opts must not be NULL'),
    ('bp_state', 'null_opts', 1, 'opts must not be NULL'),
    ('dantzig', 'null_opts', 1, 'opts must not be NULL'),
    ('dantzig_traced', 'null_opts', 1, 'opts must not be NULL'),
    ('parbp', 'null_opts', 1, 'opts must not be NULL'),
    ('parbp_traced', 'null_opts', 1, 'opts must not be NULL'),
    ('parbp_dist', 'null_opts', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso_plan_create_dist', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso_plan_create_dist_cols', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso_dist', 'null_opts', 1, 'opts must not be NULL'),
    ('parlasso_dist', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso_dist_cols', 'null_opts', 1, 'opts must not be NULL'),
    ('lasso', 'maxit_zero', 1, 'maxit should be positive'),
    ('enet', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso_cv', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso_multi', 'maxit_zero', 1, 'maxit should be positive'),
    ('parlasso', 'maxit_zero', 1, 'maxit should be positive'),
    ('lad', 'maxit_zero', 1, 'maxit should be positive'),
    ('lad_traced', 'maxit_zero', 1, 'maxit should be positive'),
    ('lad_state', 'maxit_zero', 1, 'maxit should be positive'),
    ('bp', 'maxit_zero', 1, 'maxit should be positive'),
    ('bp_traced', 'maxit_zero', 1, 'maxit should be positive'),
    ('bp_state', 'maxit_zero', 1, 'maxit should be positive'),
    ('dantzig', 'maxit_zero', 1, 'maxit should be positive'),
    ('dantzig_traced', 'maxit_zero', 1, 'maxit should be positive'),
    ('parbp', 'maxit_zero', 1, 'maxit should be positive'),
    ('parbp_traced', 'maxit_zero', 1, 'maxit should be positive'),
    ('parbp_dist', 'maxit_zero', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso_plan_create_dist', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso_plan_create_dist_cols', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso_dist', 'maxit_zero', 1, 'maxit should be positive'),
    ('parlasso_dist', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso_dist_cols', 'maxit_zero', 1, 'maxit should be positive'),
    ('lasso', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('enet', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso_cv', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso_multi', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('parlasso', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lad', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lad_traced', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lad_state', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('bp', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('bp_traced', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('bp_state', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('dantzig', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('dantzig_traced', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('parbp', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('parbp_traced', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('parbp_dist', 'neg_eps', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso_plan_create_dist', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso_plan_create_dist_cols', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso_dist', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('parlasso_dist', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso_dist_cols', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('lasso', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('enet', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso_cv', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),  # was NO_DEVICE without a GPU: the grid was checked after the upload; with a GPU the same code and text as before
    ('lasso_multi', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('parlasso', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('dantzig', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('dantzig_traced', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso_plan_create', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso_plan_create_dist', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso_plan_create_dist_cols', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso_dist', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('parlasso_dist', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso_dist_cols', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('lasso', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('enet', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso_cv', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),  # was NO_DEVICE without a GPU: the grid was checked after the upload; with a GPU the same code and text as before
    ('lasso_multi', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('parlasso', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('dantzig', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('dantzig_traced', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso_plan_create', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso_plan_create_dist', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso_plan_create_dist_cols', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso_dist', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('parlasso_dist', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso_dist_cols', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('lasso', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('enet', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso_cv', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),  # was NO_DEVICE without a GPU: the grid was checked after the upload; with a GPU the same code and text as before
    ('lasso_multi', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),  # was NO_DEVICE without a GPU: the grid was checked after the upload; with a GPU the same code and text as before
    ('parlasso', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('dantzig', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('dantzig_traced', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso_plan_create', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso_plan_create_dist', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso_plan_create_dist_cols', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso_dist', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('parlasso_dist', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso_dist_cols', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('lasso', 'neg_lambda', 1, 'lambda must be positive'),
    ('enet', 'neg_lambda', 1, 'lambda must be positive'),
    ('lasso_cv', 'neg_lambda', 1, 'lambda must be positive'),  # was NO_DEVICE without a GPU: the grid was checked after the upload; with a GPU the same code and text as before
    ('lasso_multi', 'neg_lambda', 1, 'lambda must be positive'),  # was NO_DEVICE without a GPU: the grid was checked after the upload; with a GPU the same code and text as before
    ('parlasso', 'neg_lambda', 1, 'lambda must be positive'),
    ('dantzig', 'neg_lambda', 1, 'lambda must be positive'),
    ('dantzig_traced', 'neg_lambda', 1, 'lambda must be positive'),
    ('lasso_plan_create', 'neg_lambda', 1, 'lambda must be positive'),
    ('lasso_plan_create_dist', 'neg_lambda', 1, 'lambda must be positive'),
    ('lasso_plan_create_dist_cols', 'neg_lambda', 1, 'lambda must be positive'),
    ('lasso_dist', 'neg_lambda', 1, 'lambda must be positive'),
    ('parlasso_dist', 'neg_lambda', 1, 'lambda must be positive'),
    ('lasso_dist_cols', 'neg_lambda', 1, 'lambda must be positive'),
    ('enet', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('lasso_cv', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('lasso_multi', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('lasso_plan_create', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('lasso_plan_create_dist_cols', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('lasso_dist', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('lasso_dist_cols', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('enet', 'alpha_neg', 1, 'alpha must be within [0, 1]'),
    ('lasso', 'null_out', 1, 'output pointers must not be NULL'),
    ('enet', 'null_out', 1, 'output pointers must not be NULL'),
    ('lasso_cv', 'null_out', 1, 'lambda_out, cv_mean and cv_se must not be NULL'),
    ('lasso_multi', 'null_out', 1, 'output pointers must not be NULL'),
    ('parlasso', 'null_out', 1, 'output pointers must not be NULL'),
    ('lad', 'null_out', 1, 'output pointers must not be NULL'),
    ('lad_traced', 'null_out', 1, 'output pointers must not be NULL'),
    ('lad_state', 'null_out', 1, 'output pointers must not be NULL'),
    ('bp', 'null_out', 1, 'output pointers must not be NULL'),
    ('bp_traced', 'null_out', 1, 'output pointers must not be NULL'),
    ('bp_state', 'null_out', 1, 'output pointers must not be NULL'),
    ('dantzig', 'null_out', 1, 'output pointers must not be NULL'),
    ('dantzig_traced', 'null_out', 1, 'output pointers must not be NULL'),
    ('parbp', 'null_out', 1, 'output pointers must not be NULL'),
    ('parbp_traced', 'null_out', 1, 'output pointers must not be NULL'),
    ('parbp_dist', 'null_out', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'null_out', 1, 'plan_out must not be NULL'),
    ('lasso_plan_create_dist', 'null_out', 1, 'plan_out must not be NULL'),
    ('lasso_plan_create_dist_cols', 'null_out', 1, 'plan_out must not be NULL'),
    ('lasso_dist', 'null_out', 1, 'output pointers must not be NULL'),
    ('parlasso_dist', 'null_out', 1, 'output pointers must not be NULL'),
    ('lasso_dist_cols', 'null_out', 1, 'output pointers must not be NULL'),
    ('lad_traced', 'trace_null', 1, 'bad trace arguments'),
    ('lad_state', 'trace_null', 1, 'bad trace arguments'),
    ('bp_traced', 'trace_null', 1, 'bad trace arguments'),
    ('bp_state', 'trace_null', 1, 'bad trace arguments'),
    ('dantzig_traced', 'trace_null', 1, 'bad trace arguments'),
    ('parbp_traced', 'trace_null', 1, 'bad trace arguments'),
    ('lad_state', 'state_no_trace', 1, 'bad state arguments (the iterate dump needs the trace)'),
    ('bp_state', 'state_no_trace', 1, 'bad state arguments (the iterate dump needs the trace)'),
    ('lad', 'rho_zero', 1, 'rho should be positive'),
    ('lad_traced', 'rho_zero', 1, 'rho should be positive'),
    ('lad_state', 'rho_zero', 1, 'rho should be positive'),
    ('bp', 'rho_zero', 1, 'rho should be positive'),
    ('bp_traced', 'rho_zero', 1, 'rho should be positive'),
    ('bp_state', 'rho_zero', 1, 'rho should be positive'),
    ('parbp', 'rho_zero', 1, 'rho should be positive'),
    ('parbp_traced', 'rho_zero', 1, 'rho should be positive'),
    ('parbp_dist', 'rho_zero', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lad', 'lad_wide', 1, 'nrow(x) must be greater than ncol(x)'),
    ('lad_traced', 'lad_wide', 1, 'nrow(x) must be greater than ncol(x)'),
    ('lad_state', 'lad_wide', 1, 'nrow(x) must be greater than ncol(x)'),
    ('bp', 'bp_tall', 1, 'ncol(x) must be greater than nrow(x)'),
    ('bp_traced', 'bp_tall', 1, 'ncol(x) must be greater than nrow(x)'),
    ('bp_state', 'bp_tall', 1, 'ncol(x) must be greater than nrow(x)'),
    ('parbp', 'bp_tall', 1, 'ncol(x) must be greater than nrow(x)'),
    ('parbp_traced', 'bp_tall', 1, 'ncol(x) must be greater than nrow(x)'),
    ('dantzig', 'dantzig_p2', 1, 'the spectral-radius estimate needs at least 3 columns'),
    ('dantzig_traced', 'dantzig_p2', 1, 'the spectral-radius estimate needs at least 3 columns'),
    ('parlasso', 'nthread_zero', 1, 'nthread must be >= 1'),
    ('parbp', 'nthread_zero', 1, 'nthread must be within [1, ncol(x)]'),
    ('parbp_traced', 'nthread_zero', 1, 'nthread must be within [1, ncol(x)]'),
    ('parbp_dist', 'nthread_zero', 1, 'no communicator: call admm_hip_comm_init first'),
    ('parlasso', 'nthread_big', 1, 'more row blocks than rows'),
    ('parbp', 'nthread_big', 1, 'nthread must be within [1, ncol(x)]'),
    ('parbp_traced', 'nthread_big', 1, 'nthread must be within [1, ncol(x)]'),
    ('parbp_dist', 'nthread_big', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create', 'nthread_big', 1, 'more row blocks than rows'),
    ('lasso_cv', 'nfolds_one', 1, 'nfolds must be within [2, n]'),
    ('lasso_cv', 'fold_id_bad', 1, 'fold_id entries must be within [0, nfolds)'),  # was NO_DEVICE without a GPU: the fold checks sat behind the device check; with a GPU the same code and text as before
    ('lasso_multi', 'm_zero', 1, 'the number of responses must be >= 1'),
    ('parbp_dist', 'col_block', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create_dist_cols', 'col_block', 1, 'column block outside [0, p_total)'),
    ('lasso_dist_cols', 'col_block', 1, 'column block outside [0, p_total)'),
    ('lasso_plan_create_dist', 'n_total_small', 1, 'n_total must be >= n_local > 0'),
    ('lasso_dist', 'n_total_small', 1, 'n_total must be >= n_local > 0'),
    ('parlasso_dist', 'n_total_small', 1, 'n_total must be >= n_local > 0'),
    ('parbp_dist', 'no_comm', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create_dist', 'no_comm', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_plan_create_dist_cols', 'no_comm', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_dist', 'no_comm', 1, 'no communicator: call admm_hip_comm_init first'),
    ('parlasso_dist', 'no_comm', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso_dist_cols', 'no_comm', 1, 'no communicator: call admm_hip_comm_init first'),
    ('lasso', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('enet', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_cv', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_multi', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('parlasso', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('dantzig', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('dantzig_traced', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_plan_create', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_plan_create_dist', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_plan_create_dist_cols', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_dist', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('parlasso_dist', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('lasso_dist_cols', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
]


def _pointer(a, ctype=None):
    return a.ctypes.data if ctype is None else a.ctypes.data_as(ctypes.POINTER(ctype))


def _call(lib, entry, overrides):
    """One call of admm_hip_<entry> on 4 x 2 data, well formed but for `overrides`; returns (code, message)."""
    from admm_amd._lib import AdmmOpts
    n, p = SHAPES.get(entry, (4, 2))
    keep = {"x": np.asfortranarray(np.arange(8.0).reshape(4, 2) % 3), "y": np.ones(4), "lambda_out": np.zeros(16), "beta_out": np.zeros(64, np.float32),
            "dbeta_out": np.zeros(64), "niter_out": np.zeros(16, np.int32), "cv_mean": np.zeros(16), "cv_se": np.zeros(16),
            "trace_out": np.zeros(64), "state_out": np.zeros(64), "ntrace_out": ctypes.c_longlong(), "nstate_out": ctypes.c_longlong(),
            "plan_out": ctypes.c_void_p()}
    v = dict(x=_pointer(keep["x"]), y=_pointer(keep["y"]), n=n, p=p, m=1, mem=0, lambda_in=None, nlambda_in=0, nlambda_auto=2, lmin_ratio=0.5,
             standardize=1, intercept=1, alpha=0.5, nthread=2, fold_id=None, nfolds=2, n_total=8, p_total=8, col_offset=0,
             opts=(10, 1e-5, 1e-5, 1.0), lambda_out=_pointer(keep["lambda_out"], ctypes.c_double), beta_out=_pointer(keep["beta_out"], ctypes.c_float),
             dbeta_out=_pointer(keep["dbeta_out"], ctypes.c_double), niter_out=_pointer(keep["niter_out"], ctypes.c_int), stats=None,
             cv_mean=_pointer(keep["cv_mean"], ctypes.c_double), cv_se=_pointer(keep["cv_se"], ctypes.c_double), fold_mse=None, fold_niter=None,
             fold_beta=None, idx_min=None, idx_1se=None, trace_out=None, trace_cap=0, ntrace_out=None, state_out=None, state_cap=0, nstate_out=None,
             plan_out=ctypes.byref(keep["plan_out"]), nlambda_out=None)
    if entry in ("lasso_plan_create", "parlasso_dist", "lasso_plan_create_dist"):
        v["alpha"], v["nthread"] = -1.0, (0 if entry == "lasso_plan_create" else 2)
    v.update(overrides)
    if v["trace_cap"] > 0 or v["state_cap"] > 0:                     # buffers go with a capacity unless the rule takes them away
        for cap, buf, cnt in (("trace_cap", "trace_out", "ntrace_out"), ("state_cap", "state_out", "nstate_out")):
            if buf not in overrides:
                v[buf], v[cnt] = _pointer(keep[buf], ctypes.c_double), ctypes.byref(keep[cnt])
    if isinstance(v["opts"], tuple):
        keep["opts"] = AdmmOpts(*v["opts"])
        v["opts"] = ctypes.byref(keep["opts"])
    if v["lambda_in"] is not None:
        keep["lambda_in"] = np.array(v["lambda_in"], dtype=np.float64)
        v["lambda_in"] = _pointer(keep["lambda_in"])
    if v["fold_id"] is not None:
        keep["fold_id"] = np.array(v["fold_id"], dtype=np.int32)
        v["fold_id"] = _pointer(keep["fold_id"], ctypes.c_int)
    rc = getattr(lib, "admm_hip_" + entry)(*[v[name] for name in SIGNATURES[entry].split()])
    assert keep["plan_out"].value is None or rc == 0
    return rc, lib.admm_hip_last_error().decode()


def observe(lib):
    """The table as `lib` answers it (how TABLE was recorded)."""
    return [(e, r) + _call(lib, e, RULES[r]) for r in RULES for e in CONCERNS[r]]


def test_the_table_covers_every_rule_for_every_entry_point_it_concerns():
    assert sorted((e, r) for e, r, _, _ in TABLE) == sorted((e, r) for r in RULES for e in CONCERNS[r])
    assert len(SIGNATURES) == 22 and all(code == INVALID_ARG for _, _, code, _ in TABLE)


@pytest.mark.parametrize("entry", list(SIGNATURES))
def test_bad_calls_are_refused_with_the_recorded_code_and_message(entry):
    from admm_amd import _lib
    lib = _lib.load()
    rows = [t for t in TABLE if t[0] == entry]
    assert len(rows) >= 7
    for _, rule, code, message in rows:
        assert _call(lib, entry, RULES[rule]) == (code, message), (entry, rule)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_well_formed_calls_pass_every_check_and_then_find_no_device():
    """Nothing is dereferenced early and no check misfires: a good call gets as far as the device.  The _dist entry points cannot
    (attaching a communicator needs a device): their good call is the `no_comm` row of the table."""
    from admm_amd import _lib
    lib = _lib.load()
    for entry in SIGNATURES:
        if entry not in DIST:
            assert _call(lib, entry, {})[0] == NO_DEVICE, (entry, lib.admm_hip_last_error())
