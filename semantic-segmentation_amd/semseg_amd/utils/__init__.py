"""Device-side pieces of the reference's evaluation loop (utils/trnval_utils.py, utils/misc.py)."""
from .eval_tail import (confusion_matrix, fast_hist, eval_tail, eval_minibatch, flip_tensor,   # noqa: F401
                        resize_tensor, validate_topn, EvalTailResult)
from .f_boundary import (boundary_radius, boundary_counts, f_scores, eval_mask_boundary,   # noqa: F401
                         BoundaryMeter)
