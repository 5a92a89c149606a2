from .auc import AUC_CALLS, auc_batch  # noqa: F401
from .ranking import RANK_EVAL_CALLS, ranking_measures_batch  # noqa: F401
