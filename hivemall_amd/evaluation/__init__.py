from .ranking import RANK_EVAL_CALLS, ranking_measures_batch  # noqa: F401
