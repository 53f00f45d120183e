"""What the C ABI refuses, pinned without a GPU: one bad call per rule and entry point, with the exact return code and
admm_hip_last_error() text.  Every argument check of the library runs before it looks for a device, so all of this is observable
on a machine without one.  The expected strings in TABLE are literals recorded from the library as it was before the entry points
were rebuilt on call_args.h (the rows that were allowed to change are marked), those of the group, sparse-group, box and multi-task
entry points from the library as it was before their selectors became one Penalty; they are not read from the code under test."""
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
_GROUP = "group group_weight ngroups"
_BOX = "lower upper penalty_factor"
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
    "grplasso": f"x y n p mem {_GROUP} {_PATH} opts {_OUT}",
    "grplasso_plan_create": f"x y n p mem {_GROUP} {_PATH} opts plan_out nlambda_out",
    "sgl": f"x y n p mem {_GROUP} l1_weight alpha {_PATH} opts {_OUT}",
    "sgl_plan_create": f"x y n p mem {_GROUP} l1_weight alpha {_PATH} opts plan_out nlambda_out",
    "boxenet": f"x y n p mem {_BOX} alpha {_PATH} opts {_OUT}",
    "boxenet_plan_create": f"x y n p mem {_BOX} alpha {_PATH} opts plan_out nlambda_out",
    "mtlasso": f"x y n p m mem row_weight {_PATH} opts {_OUT}",
    "mtlasso_plan_create": f"x y n p m mem row_weight {_PATH} opts plan_out nlambda_out",
}
# the 8 doubles of x are read as 4 x 2 by default; BP, ParBP and Dantzig need more columns than that and read them as 2 x 4
SHAPES = {e: (2, 4) for e in ("bp", "bp_traced", "bp_state", "dantzig", "dantzig_traced", "parbp", "parbp_traced", "parbp_dist")}
GROUPED = ("grplasso", "grplasso_plan_create", "sgl", "sgl_plan_create")
SGL, BOX, MT = GROUPED[2:], ("boxenet", "boxenet_plan_create"), ("mtlasso", "mtlasso_plan_create")
PENALTY = GROUPED + BOX + MT                # the tall-only penalties: 4 x 2 data, the grouping (0, 1), NULL weights and bounds, m = 1
DIST = ("parbp_dist", "lasso_plan_create_dist", "lasso_plan_create_dist_cols", "lasso_dist", "parlasso_dist", "lasso_dist_cols")

# rule -> the arguments it spoils.  opts: (maxit, eps_abs, eps_rel, rho); lambda_in: the grid's values; _options: thread options set
# around the call
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
    # the tall-only penalties: one rule per check of PathSpec::check_group_ids, check_groups, check_sgl_args, check_mt, check_box_args
    "n_le_p": dict(n=2),
    "refine": dict(_options=dict(REFINE="1")),
    "group_null": dict(group=None),
    "group_start": dict(group=(1, 1)),
    "group_decreasing": dict(group=(0, -1)),
    "group_gap": dict(group=(0, 2)),
    "group_long": dict(p=1026, group=(0,) * 1026, ngroups=1),     # (n <= p too: refused before x would be read)
    "ngroups_off": dict(ngroups=3),
    "group_weight_neg": dict(group_weight=(1.0, -1.0)),
    "group_weight_inf": dict(group_weight=(np.inf, 1.0)),
    "group_weight_zero": dict(group_weight=(0.0, 0.0)),
    "alpha_nan": dict(alpha=np.nan),
    "l1_weight_nan": dict(l1_weight=(1.0, np.nan)),
    "sgl_no_penalty": dict(alpha=0.0, group_weight=(0.0, 0.0)),
    "m_big": dict(m=17),
    "row_weight_neg": dict(row_weight=(-1.0, 1.0)),
    "row_weight_zero": dict(row_weight=(0.0, 0.0)),
    "lower_pos": dict(lower=(0.0, 0.1)),
    "upper_nan": dict(upper=(np.nan, 0.0)),
    "factor_neg": dict(penalty_factor=(1.0, -0.5)),
    "factor_zero": dict(penalty_factor=(0.0, 0.0)),
    # two faults at once: which check comes first
    "nlambda_neg+group_null": dict(nlambda_in=-1, group=None),
    "group_gap+n_le_p": dict(group=(0, 2), n=2),
    "l1_weight_nan+alpha_big": dict(l1_weight=(1.0, np.nan), alpha=1.5),
    "group_weight_neg+l1_weight_nan": dict(group_weight=(1.0, -1.0), l1_weight=(1.0, np.nan)),
    "m_big+row_weight_neg": dict(m=17, row_weight=(-1.0, 1.0)),
    "row_weight_neg+n_le_p": dict(row_weight=(-1.0, 1.0), n=2),
    "upper_nan+lower_pos": dict(upper=(np.nan, 0.0), lower=(0.0, 0.1)),
    "factor_neg+alpha_nan": dict(penalty_factor=(1.0, -0.5), alpha=np.nan),
    "null_out+upper_nan": dict(lambda_out=None, plan_out=None, upper=(np.nan, 0.0)),
    "n_le_p+refine": dict(n=2, _options=dict(REFINE="1")),
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
    "m_zero": ["lasso_multi", *MT],
    "col_block": ["parbp_dist", "lasso_plan_create_dist_cols", "lasso_dist_cols"],
    "n_total_small": ["lasso_plan_create_dist", "lasso_dist", "parlasso_dist"],
    "no_comm": list(DIST),
    **{r: list(PENALTY) for r in ("n_le_p", "refine", "n_le_p+refine")},
    **{r: list(GROUPED) for r in ("group_null", "group_start", "group_decreasing", "group_gap", "group_long", "ngroups_off", "group_weight_neg",
                                  "group_weight_inf", "nlambda_neg+group_null", "group_gap+n_le_p")},
    "group_weight_zero": list(GROUPED[:2]),               # (the sparse-group call still has its l1 part: sgl_no_penalty)
    "alpha_nan": [*SGL, *BOX],
    **{r: list(SGL) for r in ("l1_weight_nan", "sgl_no_penalty", "l1_weight_nan+alpha_big", "group_weight_neg+l1_weight_nan")},
    **{r: list(MT) for r in ("m_big", "row_weight_neg", "row_weight_zero", "m_big+row_weight_neg", "row_weight_neg+n_le_p")},
    **{r: list(BOX) for r in ("lower_pos", "upper_nan", "factor_neg", "factor_zero", "upper_nan+lower_pos", "factor_neg+alpha_nan",
                              "null_out+upper_nan")},
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
    # the eight entry points of the tall-only penalties, recorded before PathSpec got its one Penalty selector
    ('grplasso', 'null_x', 1, 'x and y must not be NULL'),
    ('grplasso_plan_create', 'null_x', 1, 'x and y must not be NULL'),
    ('sgl', 'null_x', 1, 'x and y must not be NULL'),
    ('sgl_plan_create', 'null_x', 1, 'x and y must not be NULL'),
    ('boxenet', 'null_x', 1, 'x and y must not be NULL'),
    ('boxenet_plan_create', 'null_x', 1, 'x and y must not be NULL'),
    ('mtlasso', 'null_x', 1, 'x and y must not be NULL'),
    ('mtlasso_plan_create', 'null_x', 1, 'x and y must not be NULL'),
    ('grplasso', 'n_zero', 1, 'n and p must be positive'),
    ('grplasso_plan_create', 'n_zero', 1, 'n and p must be positive'),
    ('sgl', 'n_zero', 1, 'n and p must be positive'),
    ('sgl_plan_create', 'n_zero', 1, 'n and p must be positive'),
    ('boxenet', 'n_zero', 1, 'n and p must be positive'),
    ('boxenet_plan_create', 'n_zero', 1, 'n and p must be positive'),
    ('mtlasso', 'n_zero', 1, 'n and p must be positive'),
    ('mtlasso_plan_create', 'n_zero', 1, 'n and p must be positive'),
    ('grplasso', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('grplasso_plan_create', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('sgl', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('sgl_plan_create', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('boxenet', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('boxenet_plan_create', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('mtlasso', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('mtlasso_plan_create', 'bad_mem', 1, 'mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE'),
    ('grplasso', 'null_opts', 1, 'opts must not be NULL'),
    ('grplasso_plan_create', 'null_opts', 1, 'opts must not be NULL'),
    ('sgl', 'null_opts', 1, 'opts must not be NULL'),
    ('sgl_plan_create', 'null_opts', 1, 'opts must not be NULL'),
    ('boxenet', 'null_opts', 1, 'opts must not be NULL'),
    ('boxenet_plan_create', 'null_opts', 1, 'opts must not be NULL'),
    ('mtlasso', 'null_opts', 1, 'opts must not be NULL'),
    ('mtlasso_plan_create', 'null_opts', 1, 'opts must not be NULL'),
    ('grplasso', 'maxit_zero', 1, 'maxit should be positive'),
    ('grplasso_plan_create', 'maxit_zero', 1, 'maxit should be positive'),
    ('sgl', 'maxit_zero', 1, 'maxit should be positive'),
    ('sgl_plan_create', 'maxit_zero', 1, 'maxit should be positive'),
    ('boxenet', 'maxit_zero', 1, 'maxit should be positive'),
    ('boxenet_plan_create', 'maxit_zero', 1, 'maxit should be positive'),
    ('mtlasso', 'maxit_zero', 1, 'maxit should be positive'),
    ('mtlasso_plan_create', 'maxit_zero', 1, 'maxit should be positive'),
    ('grplasso', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('grplasso_plan_create', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('sgl', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('sgl_plan_create', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('boxenet', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('boxenet_plan_create', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('mtlasso', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('mtlasso_plan_create', 'neg_eps', 1, 'eps_abs and eps_rel should be nonnegative'),
    ('grplasso', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('grplasso_plan_create', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('sgl', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('sgl_plan_create', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('boxenet', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('boxenet_plan_create', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('mtlasso', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('mtlasso_plan_create', 'nlambda_neg', 1, 'nlambda_in must be >= 0'),
    ('grplasso', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('grplasso_plan_create', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('sgl', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('sgl_plan_create', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('boxenet', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('boxenet_plan_create', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('mtlasso', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('mtlasso_plan_create', 'no_grid', 1, 'need a lambda grid or nlambda_auto > 0'),
    ('grplasso', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('grplasso_plan_create', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('sgl', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('sgl_plan_create', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('boxenet', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('boxenet_plan_create', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('mtlasso', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('mtlasso_plan_create', 'lmin_one', 1, 'lambda_min_ratio must be within (0, 1)'),
    ('grplasso', 'neg_lambda', 1, 'lambda must be positive'),
    ('grplasso_plan_create', 'neg_lambda', 1, 'lambda must be positive'),
    ('sgl', 'neg_lambda', 1, 'lambda must be positive'),
    ('sgl_plan_create', 'neg_lambda', 1, 'lambda must be positive'),
    ('boxenet', 'neg_lambda', 1, 'lambda must be positive'),
    ('boxenet_plan_create', 'neg_lambda', 1, 'lambda must be positive'),
    ('mtlasso', 'neg_lambda', 1, 'lambda must be positive'),
    ('mtlasso_plan_create', 'neg_lambda', 1, 'lambda must be positive'),
    ('sgl', 'alpha_big', 1, 'the mixing parameter alpha must be finite and within [0, 1]'),
    ('sgl_plan_create', 'alpha_big', 1, 'the mixing parameter alpha must be finite and within [0, 1]'),
    ('boxenet', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('boxenet_plan_create', 'alpha_big', 1, 'alpha must be within [0, 1]'),
    ('grplasso', 'null_out', 1, 'output pointers must not be NULL'),
    ('grplasso_plan_create', 'null_out', 1, 'plan_out must not be NULL'),
    ('sgl', 'null_out', 1, 'output pointers must not be NULL'),
    ('sgl_plan_create', 'null_out', 1, 'plan_out must not be NULL'),
    ('boxenet', 'null_out', 1, 'output pointers must not be NULL'),
    ('boxenet_plan_create', 'null_out', 1, 'plan_out must not be NULL'),
    ('mtlasso', 'null_out', 1, 'output pointers must not be NULL'),
    ('mtlasso_plan_create', 'null_out', 1, 'plan_out must not be NULL'),
    ('mtlasso', 'm_zero', 1, 'the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]'),
    ('mtlasso_plan_create', 'm_zero', 1, 'the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]'),
    ('grplasso', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('grplasso_plan_create', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('sgl', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('sgl_plan_create', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('boxenet', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('boxenet_plan_create', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('mtlasso', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('mtlasso_plan_create', 'maxit_zero+nlambda_neg', 1, 'maxit should be positive'),
    ('grplasso', 'n_le_p', 1, 'the group lasso is built for n > p only'),
    ('grplasso_plan_create', 'n_le_p', 1, 'the group lasso is built for n > p only'),
    ('sgl', 'n_le_p', 1, 'the sparse-group lasso is built for n > p only'),
    ('sgl_plan_create', 'n_le_p', 1, 'the sparse-group lasso is built for n > p only'),
    ('boxenet', 'n_le_p', 1, 'the box-constrained elastic net is built for n > p only: the wide solver is not built for bounds'),
    ('boxenet_plan_create', 'n_le_p', 1, 'the box-constrained elastic net is built for n > p only: the wide solver is not built for bounds'),
    ('mtlasso', 'n_le_p', 1, 'the multi-task lasso is built for n > p only'),
    ('mtlasso_plan_create', 'n_le_p', 1, 'the multi-task lasso is built for n > p only'),
    ('grplasso', 'refine', 1, 'the group lasso has no refined x-update: unset REFINE'),
    ('grplasso_plan_create', 'refine', 1, 'the group lasso has no refined x-update: unset REFINE'),
    ('sgl', 'refine', 1, 'the group lasso has no refined x-update: unset REFINE'),
    ('sgl_plan_create', 'refine', 1, 'the group lasso has no refined x-update: unset REFINE'),
    ('boxenet', 'refine', 1, 'the box-constrained elastic net has no refined x-update: unset REFINE'),
    ('boxenet_plan_create', 'refine', 1, 'the box-constrained elastic net has no refined x-update: unset REFINE'),
    ('mtlasso', 'refine', 1, 'the multi-task lasso has no refined x-update: unset REFINE'),
    ('mtlasso_plan_create', 'refine', 1, 'the multi-task lasso has no refined x-update: unset REFINE'),
    ('grplasso', 'group_null', 1, 'group must not be NULL'),
    ('grplasso_plan_create', 'group_null', 1, 'group must not be NULL'),
    ('sgl', 'group_null', 1, 'group must not be NULL'),
    ('sgl_plan_create', 'group_null', 1, 'group must not be NULL'),
    ('grplasso', 'group_start', 1, 'group ids must start at 0'),
    ('grplasso_plan_create', 'group_start', 1, 'group ids must start at 0'),
    ('sgl', 'group_start', 1, 'group ids must start at 0'),
    ('sgl_plan_create', 'group_start', 1, 'group ids must start at 0'),
    ('grplasso', 'group_decreasing', 1, 'group ids must be non-decreasing (the columns of a group are adjacent)'),
    ('grplasso_plan_create', 'group_decreasing', 1, 'group ids must be non-decreasing (the columns of a group are adjacent)'),
    ('sgl', 'group_decreasing', 1, 'group ids must be non-decreasing (the columns of a group are adjacent)'),
    ('sgl_plan_create', 'group_decreasing', 1, 'group ids must be non-decreasing (the columns of a group are adjacent)'),
    ('grplasso', 'group_gap', 1, 'group ids must have no gaps'),
    ('grplasso_plan_create', 'group_gap', 1, 'group ids must have no gaps'),
    ('sgl', 'group_gap', 1, 'group ids must have no gaps'),
    ('sgl_plan_create', 'group_gap', 1, 'group ids must have no gaps'),
    ('grplasso', 'group_long', 1, 'a group has more than ADMM_HIP_GROUP_MAX (1024) columns'),
    ('grplasso_plan_create', 'group_long', 1, 'a group has more than ADMM_HIP_GROUP_MAX (1024) columns'),
    ('sgl', 'group_long', 1, 'a group has more than ADMM_HIP_GROUP_MAX (1024) columns'),
    ('sgl_plan_create', 'group_long', 1, 'a group has more than ADMM_HIP_GROUP_MAX (1024) columns'),
    ('grplasso', 'ngroups_off', 1, 'ngroups does not match the group ids'),
    ('grplasso_plan_create', 'ngroups_off', 1, 'ngroups does not match the group ids'),
    ('sgl', 'ngroups_off', 1, 'ngroups does not match the group ids'),
    ('sgl_plan_create', 'ngroups_off', 1, 'ngroups does not match the group ids'),
    ('grplasso', 'group_weight_neg', 1, 'group weights must be finite and non-negative'),
    ('grplasso_plan_create', 'group_weight_neg', 1, 'group weights must be finite and non-negative'),
    ('sgl', 'group_weight_neg', 1, 'group weights must be finite and non-negative'),
    ('sgl_plan_create', 'group_weight_neg', 1, 'group weights must be finite and non-negative'),
    ('grplasso', 'group_weight_inf', 1, 'group weights must be finite and non-negative'),
    ('grplasso_plan_create', 'group_weight_inf', 1, 'group weights must be finite and non-negative'),
    ('sgl', 'group_weight_inf', 1, 'group weights must be finite and non-negative'),
    ('sgl_plan_create', 'group_weight_inf', 1, 'group weights must be finite and non-negative'),
    ('grplasso', 'group_weight_zero', 1, 'at least one group weight must be positive'),
    ('grplasso_plan_create', 'group_weight_zero', 1, 'at least one group weight must be positive'),
    ('sgl', 'alpha_nan', 1, 'the mixing parameter alpha must be finite and within [0, 1]'),
    ('sgl_plan_create', 'alpha_nan', 1, 'the mixing parameter alpha must be finite and within [0, 1]'),
    ('boxenet', 'alpha_nan', 1, "alpha must be negative (the Lasso prox) or within [0, 1] (the elastic net's)"),
    ('boxenet_plan_create', 'alpha_nan', 1, "alpha must be negative (the Lasso prox) or within [0, 1] (the elastic net's)"),
    ('sgl', 'l1_weight_nan', 1, 'l1 weights must be finite and non-negative'),
    ('sgl_plan_create', 'l1_weight_nan', 1, 'l1 weights must be finite and non-negative'),
    ('sgl', 'sgl_no_penalty', 1, 'at least one coordinate must carry a positive penalty'),
    ('sgl_plan_create', 'sgl_no_penalty', 1, 'at least one coordinate must carry a positive penalty'),
    ('mtlasso', 'm_big', 1, 'the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]'),
    ('mtlasso_plan_create', 'm_big', 1, 'the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]'),
    ('mtlasso', 'row_weight_neg', 1, 'row weights must be finite and non-negative'),
    ('mtlasso_plan_create', 'row_weight_neg', 1, 'row weights must be finite and non-negative'),
    ('mtlasso', 'row_weight_zero', 1, 'at least one row weight must be positive'),
    ('mtlasso_plan_create', 'row_weight_zero', 1, 'at least one row weight must be positive'),
    ('boxenet', 'lower_pos', 1, 'lower bounds must be <= 0 (zero must be feasible) and not NaN'),
    ('boxenet_plan_create', 'lower_pos', 1, 'lower bounds must be <= 0 (zero must be feasible) and not NaN'),
    ('boxenet', 'upper_nan', 1, 'upper bounds must be >= 0 (zero must be feasible) and not NaN'),
    ('boxenet_plan_create', 'upper_nan', 1, 'upper bounds must be >= 0 (zero must be feasible) and not NaN'),
    ('boxenet', 'factor_neg', 1, 'penalty factors must be finite and non-negative'),
    ('boxenet_plan_create', 'factor_neg', 1, 'penalty factors must be finite and non-negative'),
    ('boxenet', 'factor_zero', 1, 'at least one penalty factor must be positive'),
    ('boxenet_plan_create', 'factor_zero', 1, 'at least one penalty factor must be positive'),
    ('grplasso', 'nlambda_neg+group_null', 1, 'nlambda_in must be >= 0'),
    ('grplasso_plan_create', 'nlambda_neg+group_null', 1, 'nlambda_in must be >= 0'),
    ('sgl', 'nlambda_neg+group_null', 1, 'nlambda_in must be >= 0'),
    ('sgl_plan_create', 'nlambda_neg+group_null', 1, 'nlambda_in must be >= 0'),
    ('grplasso', 'group_gap+n_le_p', 1, 'group ids must have no gaps'),
    ('grplasso_plan_create', 'group_gap+n_le_p', 1, 'group ids must have no gaps'),
    ('sgl', 'group_gap+n_le_p', 1, 'group ids must have no gaps'),
    ('sgl_plan_create', 'group_gap+n_le_p', 1, 'group ids must have no gaps'),
    ('sgl', 'l1_weight_nan+alpha_big', 1, 'the mixing parameter alpha must be finite and within [0, 1]'),
    ('sgl_plan_create', 'l1_weight_nan+alpha_big', 1, 'the mixing parameter alpha must be finite and within [0, 1]'),
    ('sgl', 'group_weight_neg+l1_weight_nan', 1, 'group weights must be finite and non-negative'),
    ('sgl_plan_create', 'group_weight_neg+l1_weight_nan', 1, 'group weights must be finite and non-negative'),
    ('mtlasso', 'm_big+row_weight_neg', 1, 'the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]'),
    ('mtlasso_plan_create', 'm_big+row_weight_neg', 1, 'the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]'),
    ('mtlasso', 'row_weight_neg+n_le_p', 1, 'row weights must be finite and non-negative'),
    ('mtlasso_plan_create', 'row_weight_neg+n_le_p', 1, 'row weights must be finite and non-negative'),
    ('boxenet', 'upper_nan+lower_pos', 1, 'lower bounds must be <= 0 (zero must be feasible) and not NaN'),
    ('boxenet_plan_create', 'upper_nan+lower_pos', 1, 'lower bounds must be <= 0 (zero must be feasible) and not NaN'),
    ('boxenet', 'factor_neg+alpha_nan', 1, 'penalty factors must be finite and non-negative'),
    ('boxenet_plan_create', 'factor_neg+alpha_nan', 1, 'penalty factors must be finite and non-negative'),
    ('boxenet', 'null_out+upper_nan', 1, 'output pointers must not be NULL'),
    ('boxenet_plan_create', 'null_out+upper_nan', 1, 'plan_out must not be NULL'),
    ('grplasso', 'n_le_p+refine', 1, 'the group lasso is built for n > p only'),
    ('grplasso_plan_create', 'n_le_p+refine', 1, 'the group lasso is built for n > p only'),
    ('sgl', 'n_le_p+refine', 1, 'the sparse-group lasso is built for n > p only'),
    ('sgl_plan_create', 'n_le_p+refine', 1, 'the sparse-group lasso is built for n > p only'),
    ('boxenet', 'n_le_p+refine', 1, 'the box-constrained elastic net is built for n > p only: the wide solver is not built for bounds'),
    ('boxenet_plan_create', 'n_le_p+refine', 1, 'the box-constrained elastic net is built for n > p only: the wide solver is not built for bounds'),
    ('mtlasso', 'n_le_p+refine', 1, 'the multi-task lasso is built for n > p only'),
    ('mtlasso_plan_create', 'n_le_p+refine', 1, 'the multi-task lasso is built for n > p only'),
]


def _pointer(a, ctype=None):
    return a.ctypes.data if ctype is None else a.ctypes.data_as(ctypes.POINTER(ctype))


def _call(lib, entry, overrides):
    """One call of admm_hip_<entry> on 4 x 2 data, well formed but for `overrides`; returns (code, message)."""
    from admm_amd import _lib
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
             plan_out=ctypes.byref(keep["plan_out"]), nlambda_out=None,
             group=(0, 1), group_weight=None, ngroups=2, l1_weight=None, row_weight=None, lower=None, upper=None, penalty_factor=None)
    if entry in ("lasso_plan_create", "parlasso_dist", "lasso_plan_create_dist"):
        v["alpha"], v["nthread"] = -1.0, (0 if entry == "lasso_plan_create" else 2)
    v.update(overrides)
    thread_options = v.pop("_options", {})
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
    if v["group"] is not None:
        keep["group"] = np.array(v["group"], dtype=np.int32)
        v["group"] = _pointer(keep["group"], ctypes.c_int)
    for name in ("group_weight", "l1_weight", "row_weight", "lower", "upper", "penalty_factor"):
        if v[name] is not None:
            keep[name] = np.array(v[name], dtype=np.float64)
            v[name] = _pointer(keep[name], ctypes.c_double)
    with _lib.options(**thread_options):
        rc = getattr(lib, "admm_hip_" + entry)(*[v[name] for name in SIGNATURES[entry].split()])
    assert keep["plan_out"].value is None or rc == 0
    return rc, lib.admm_hip_last_error().decode()


def observe(lib):
    """The table as `lib` answers it (how TABLE was recorded)."""
    return [(e, r) + _call(lib, e, RULES[r]) for r in RULES for e in CONCERNS[r]]


def test_the_table_covers_every_rule_for_every_entry_point_it_concerns():
    assert sorted((e, r) for e, r, _, _ in TABLE) == sorted((e, r) for r in RULES for e in CONCERNS[r])
    assert len(SIGNATURES) == 30 and all(code == INVALID_ARG for _, _, code, _ in TABLE)


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


# ---- the hooks of the shared mat-vec family (tests/test_gpu_gemv_family.py, tests/test_gpu_block_sprad.py): argument checks only
_GEMV_EX = "is_double form nrhs nt max_seg_rows lda_extra fill count m k A v from skip part_out part_capacity y_out info_out"
_GEMV_SHAPE = "gemv_t_ex hook: m and k in 1 .. 2^20, at most 2^28 elements of storage per matrix and per partial buffer"
_GEMV_SCALARS = ("gemv_t_ex hook: is_double 0 or 1, form in 0 .. 3, nrhs 1 or 2, nt in -1 .. 1, max_seg_rows >= 0, lda_extra a multiple of 32 in 0 .. 4096, "
                 "part_capacity >= 1")
_GEMV_COUNT = "gemv_t_ex hook: forms 0 and 1 take one product, form 2 two, form 3 one to eight"
_GEMV_FROM = "gemv_t_ex hook: from[i] is -1 or a product that is not chained itself and has k[from[i]] == m[i]"
# (overrides of a well-formed form-3 call of three 4 x 4 products, the message of the refusal)
GEMV_EX_TABLE = [
    (dict(m=None), "gemv_t_ex hook: m, k, A, v, part_out and info_out must not be NULL"),
    (dict(A=None), "gemv_t_ex hook: m, k, A, v, part_out and info_out must not be NULL"),
    (dict(info_out=None), "gemv_t_ex hook: m, k, A, v, part_out and info_out must not be NULL"),
    (dict(is_double=2), _GEMV_SCALARS), (dict(form=4), _GEMV_SCALARS), (dict(form=-1), _GEMV_SCALARS), (dict(nrhs=3), _GEMV_SCALARS),
    (dict(nt=2), _GEMV_SCALARS), (dict(nt=-2), _GEMV_SCALARS), (dict(max_seg_rows=-1), _GEMV_SCALARS), (dict(lda_extra=16), _GEMV_SCALARS),
    (dict(lda_extra=8192), _GEMV_SCALARS), (dict(part_capacity=0), _GEMV_SCALARS),
    (dict(nrhs=2), "gemv_t_ex hook: two right-hand sides are built for form 0 only"),
    (dict(form=0), _GEMV_COUNT), (dict(form=1), _GEMV_COUNT), (dict(form=2), _GEMV_COUNT), (dict(count=0), _GEMV_COUNT), (dict(count=9), _GEMV_COUNT),
    (dict(form=2, count=2, **{"from": (-1, 0, -1)}), "gemv_t_ex hook: from belongs to form 3 (form 2 chains its two products itself)"),
    (dict(m=(4, 0, 4)), _GEMV_SHAPE), (dict(k=(4, 4, (1 << 20) + 1)), _GEMV_SHAPE), (dict(m=(1 << 20, 4, 4), k=(1 << 20, 4, 4)), _GEMV_SHAPE),
    (dict(A_null=1), "gemv_t_ex hook: every A[i] and part_out[i] must not be NULL"),
    (dict(part_null=2), "gemv_t_ex hook: every A[i] and part_out[i] must not be NULL"),
    (dict(skip=(0, 2, 0)), "gemv_t_ex hook: skip values are 0 or 1"),
    (dict(**{"from": (-1, 3, -1)}), _GEMV_FROM), (dict(**{"from": (-1, 1, -1)}), _GEMV_FROM), (dict(**{"from": (1, 0, -1)}), _GEMV_FROM),
    (dict(k=(5, 4, 4), **{"from": (-1, 0, -1)}), _GEMV_FROM),
    (dict(v_null=0), "gemv_t_ex hook: every product that is not chained needs its v[i]"),
    (dict(form=2, count=2, m=(4, 5, 4)), "gemv_t_ex hook: a chain needs m[1] == k[0]"),
    (dict(form=1, count=1, y_out=None), "gemv_t_ex hook: forms 1 and 2 need y_out of the last product"),
    (dict(form=2, count=2, y_null=1), "gemv_t_ex hook: forms 1 and 2 need y_out of the last product"),
]
GEMV_EX_GOOD = [dict(), dict(**{"from": (-1, 0, -1)}, v_null=1), dict(form=0, count=1, nrhs=2), dict(form=1, count=1), dict(form=2, count=2, v_null=1),
                dict(is_double=1, nt=1, max_seg_rows=128, lda_extra=64, skip=(1, 0, 1))]


def _gemv_ex(lib, over):
    n = 3
    keep = [np.zeros(64) for _ in range(4 * n)]
    v = dict(is_double=0, form=3, nrhs=1, nt=-1, max_seg_rows=0, lda_extra=0, fill=0x7FC00000, count=n, m=(4,) * n, k=(4,) * n, skip=None, part_capacity=64,
             info_out=(ctypes.c_longlong * (8 * n))(), **{"from": None})
    arrays = {name: [keep[n * j + i].ctypes.data for i in range(n)] for j, name in enumerate(("A", "v", "part_out", "y_out"))}
    over = dict(over)
    for name, key in (("A", "A_null"), ("v", "v_null"), ("part_out", "part_null"), ("y_out", "y_null")):
        if key in over:
            arrays[name][over.pop(key)] = None
    v.update({name: (ctypes.c_void_p * n)(*ptrs) for name, ptrs in arrays.items()})
    v.update(over)
    for name in ("m", "k", "from", "skip"):
        if v[name] is not None:
            v[name] = (ctypes.c_int * n)(*v[name])
    rc = lib.admm_hip_test_gemv_t_ex(*[v[name] for name in _GEMV_EX.split()])
    return rc, lib.admm_hip_last_error().decode()


def test_the_gemv_family_hook_refuses_bad_requests_before_it_looks_for_a_device():
    from admm_amd import _lib
    lib = _lib.load()
    for over, message in GEMV_EX_TABLE:
        assert _gemv_ex(lib, over) == (INVALID_ARG, message), over


_WIDE_SHAPE = "wide_op hook: n and p in 1 .. 2^20, at most 2^28 elements of storage"
_SPRAD_SHAPE = "block_sprad hook: n in 1 .. 16384, p in 1 .. 2^20, at most 2^27 elements of storage"
# (hook, overrides of a well-formed call on 4 x 6 data, message)
SMALL_HOOK_TABLE = [
    ("wide_op", dict(X=None), "wide_op hook: X, v and w must not be NULL"), ("wide_op", dict(v=None), "wide_op hook: X, v and w must not be NULL"),
    ("wide_op", dict(w=None), "wide_op hook: X, v and w must not be NULL"), ("wide_op", dict(n=0), _WIDE_SHAPE), ("wide_op", dict(p=-1), _WIDE_SHAPE),
    ("wide_op", dict(n=(1 << 20) + 1), _WIDE_SHAPE), ("wide_op", dict(n=1 << 20, p=1 << 20), _WIDE_SHAPE),
    ("block_sprad", dict(A=None), "block_sprad hook: A, out and nsteps_out must not be NULL"),
    ("block_sprad", dict(out=None), "block_sprad hook: A, out and nsteps_out must not be NULL"),
    ("block_sprad", dict(nsteps_out=None), "block_sprad hook: A, out and nsteps_out must not be NULL"),
    ("block_sprad", dict(n=0), _SPRAD_SHAPE), ("block_sprad", dict(n=16385), _SPRAD_SHAPE), ("block_sprad", dict(p=0), _SPRAD_SHAPE),
    ("block_sprad", dict(n=16384, p=1 << 14), _SPRAD_SHAPE),
    ("block_sprad", dict(nblocks=0), "block_sprad hook: nblocks in 1 .. min(64, p)"), ("block_sprad", dict(nblocks=7), "block_sprad hook: nblocks in 1 .. min(64, p)"),
    ("block_sprad", dict(p=100, nblocks=65), "block_sprad hook: nblocks in 1 .. min(64, p)"),
    ("block_sprad", dict(n=8000, p=8000, nblocks=6), "block_sprad hook: the blocks must fit one batch of Lanczos runs (3 GB of Gram matrices and bases)"),
]


def _small_hook(lib, hook, over):
    keep = dict(X=np.zeros(24, np.float32), v=np.zeros(4, np.float32), w=np.zeros(4, np.float32), A=np.zeros(24), out=np.zeros(6),
                nsteps_out=np.zeros(6, np.int32))
    types = dict(X=ctypes.c_float, v=ctypes.c_float, w=ctypes.c_float, A=ctypes.c_double, out=ctypes.c_double, nsteps_out=ctypes.c_int)
    v = dict({name: _pointer(a, types[name]) for name, a in keep.items()}, n=4, p=6, nblocks=2)
    v.update(over)
    names = "X n p v w" if hook == "wide_op" else "A n p nblocks out nsteps_out"
    rc = getattr(lib, "admm_hip_test_" + hook)(*[v[name] for name in names.split()])
    return rc, lib.admm_hip_last_error().decode()


def test_the_wide_op_and_block_sprad_hooks_refuse_bad_requests_before_they_look_for_a_device():
    from admm_amd import _lib
    lib = _lib.load()
    for hook, over, message in SMALL_HOOK_TABLE:
        assert _small_hook(lib, hook, over) == (INVALID_ARG, message), (hook, over)


# ---- the hooks of the safe screens' setup kernels (tests/test_gpu_screen_prep.py): argument checks only
_WSCR_NULL = "wide_screen_prep hook: X, copy_out, s_out, rate_out and info_out must not be NULL"
_WSCR_SHAPE = "wide_screen_prep hook: n, p and nw in 1 .. 2^20, at most 2^28 elements of storage"
_WSCR_CAP = "wide_screen_prep hook: copy_capacity below p * ldh elements"
_SSCR_NULL = "sbp_screen_prep hook: A, copy_out, s_out and info_out must not be NULL"
_SSCR_SHAPE = "sbp_screen_prep hook: n and pl in 1 .. 2^20, lda_extra in 0 .. 4096, at most 2^27 elements of storage"
# (hook, overrides of a well-formed call on 4 x 6 data -- fmt 16, nw 4, capacity 48 = 6 columns of ldh 8 --, message)
SCREEN_HOOK_TABLE = [
    ("wide_screen_prep", dict(X=None), _WSCR_NULL), ("wide_screen_prep", dict(copy_out=None), _WSCR_NULL), ("wide_screen_prep", dict(s_out=None), _WSCR_NULL),
    ("wide_screen_prep", dict(rate_out=None), _WSCR_NULL), ("wide_screen_prep", dict(info_out=None), _WSCR_NULL),
    ("wide_screen_prep", dict(fmt=0), "wide_screen_prep hook: fmt is 8 or 16"), ("wide_screen_prep", dict(fmt=32), "wide_screen_prep hook: fmt is 8 or 16"),
    ("wide_screen_prep", dict(fmt=8, copy_capacity=96, scale_out=None), "wide_screen_prep hook: the 8-bit code needs scale_out"),
    ("wide_screen_prep", dict(n=0), _WSCR_SHAPE), ("wide_screen_prep", dict(n=(1 << 20) + 1), _WSCR_SHAPE), ("wide_screen_prep", dict(p=0), _WSCR_SHAPE),
    ("wide_screen_prep", dict(p=(1 << 20) + 1), _WSCR_SHAPE), ("wide_screen_prep", dict(nw=0), _WSCR_SHAPE), ("wide_screen_prep", dict(nw=-4), _WSCR_SHAPE),
    ("wide_screen_prep", dict(nw=(1 << 20) + 1), _WSCR_SHAPE), ("wide_screen_prep", dict(n=1 << 20, p=1 << 20), _WSCR_SHAPE),
    ("wide_screen_prep", dict(copy_capacity=47), _WSCR_CAP), ("wide_screen_prep", dict(copy_capacity=0), _WSCR_CAP),
    ("wide_screen_prep", dict(fmt=8, copy_capacity=95), _WSCR_CAP), ("wide_screen_prep", dict(n=9, copy_capacity=95), _WSCR_CAP),
    ("sbp_screen_prep", dict(A=None), _SSCR_NULL), ("sbp_screen_prep", dict(copy_out=None), _SSCR_NULL), ("sbp_screen_prep", dict(s_out=None), _SSCR_NULL),
    ("sbp_screen_prep", dict(info_out=None), _SSCR_NULL),
    ("sbp_screen_prep", dict(n=0), _SSCR_SHAPE), ("sbp_screen_prep", dict(n=(1 << 20) + 1), _SSCR_SHAPE), ("sbp_screen_prep", dict(p=0), _SSCR_SHAPE),
    ("sbp_screen_prep", dict(p=(1 << 20) + 1), _SSCR_SHAPE), ("sbp_screen_prep", dict(lda_extra=-8), _SSCR_SHAPE), ("sbp_screen_prep", dict(lda_extra=4104), _SSCR_SHAPE),
    ("sbp_screen_prep", dict(n=1 << 14, p=1 << 14), _SSCR_SHAPE),
    ("sbp_screen_prep", dict(copy_capacity=47), "sbp_screen_prep hook: copy_capacity below pl * ldh elements"),
    ("sbp_screen_prep", dict(n=9, copy_capacity=95), "sbp_screen_prep hook: copy_capacity below pl * ldh elements"),
]
SCREEN_HOOK_GOOD = [("wide_screen_prep", dict()), ("wide_screen_prep", dict(fmt=8, copy_capacity=96)), ("wide_screen_prep", dict(scale_out=None)),
                    ("wide_screen_prep", dict(nw=96)), ("sbp_screen_prep", dict()), ("sbp_screen_prep", dict(lda_extra=8))]


def _screen_hook(lib, hook, over):
    keep = dict(X=np.zeros(1 << 10, np.float32), A=np.zeros(1 << 10), copy_out=np.zeros(1 << 10, np.uint16), s_out=np.zeros(1 << 14, np.float32),
                scale_out=np.zeros(1 << 14, np.float32), rate_out=np.zeros(64), info_out=np.zeros(4, np.int64))
    types = dict(X=ctypes.c_float, A=ctypes.c_double, copy_out=ctypes.c_ushort, s_out=ctypes.c_float, scale_out=ctypes.c_float, rate_out=ctypes.c_double,
                 info_out=ctypes.c_longlong)
    v = dict({name: _pointer(a, types[name]) for name, a in keep.items()}, n=4, p=6, fmt=16, nw=4, lda_extra=0, pad_fill=0x7FC00000, copy_capacity=48)
    v["copy_out"] = ctypes.cast(v["copy_out"], ctypes.c_void_p)
    v.update(over)
    names = ("X n p fmt nw pad_fill copy_out copy_capacity s_out scale_out rate_out info_out" if hook == "wide_screen_prep"
             else "A n p lda_extra pad_fill copy_out copy_capacity s_out info_out")
    rc = getattr(lib, "admm_hip_test_" + hook)(*[v[name] for name in names.split()])
    return rc, lib.admm_hip_last_error().decode()


def test_the_screen_setup_hooks_refuse_bad_requests_before_they_look_for_a_device():
    from admm_amd import _lib
    lib = _lib.load()
    for hook, over, message in SCREEN_HOOK_TABLE:
        assert _screen_hook(lib, hook, over) == (INVALID_ARG, message), (hook, over)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_well_formed_screen_hook_requests_pass_every_check_and_then_find_no_device():
    from admm_amd import _lib
    lib = _lib.load()
    for hook, over in SCREEN_HOOK_GOOD:
        assert _screen_hook(lib, hook, over)[0] == NO_DEVICE, (hook, over, lib.admm_hip_last_error())


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a machine without a GPU")
def test_well_formed_hook_requests_pass_every_check_and_then_find_no_device():
    from admm_amd import _lib
    lib = _lib.load()
    for over in GEMV_EX_GOOD:
        assert _gemv_ex(lib, over)[0] == NO_DEVICE, (over, lib.admm_hip_last_error())
    for hook in ("wide_op", "block_sprad"):
        assert _small_hook(lib, hook, {})[0] == NO_DEVICE, (hook, lib.admm_hip_last_error())
