from .estimator import fep_estimator  # noqa: F401
from .bootstrap import (bootstrap, bootstrap_fep, bootstrap_fep_resampled, bootstrap_resample_indices,  # noqa: F401
                        bootstrap_resample_weights)
