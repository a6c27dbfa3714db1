"""MI355X-native SqueezeDet hot path (inference + training) behind the reference's
``nn.Module`` / ``Detector`` / ``Trainer`` surface.  See DESIGN.md.

Importing this package never touches the GPU (fork-safe); the HIP library
``csrc/libsqdhip.so`` is loaded on first use and its absence is a hard error -- there is no
CPU fallback in the product path.
"""
from . import boxes, config, synthetic  # noqa: F401
from .config import make_cfg  # noqa: F401
from .dataset_stats import compute_dataset_anchors_seed, compute_dataset_mean_and_std  # noqa: F401
from .metrics import DetectionAP, evaluate_results  # noqa: F401

__version__ = "0.1.0"

_TRAINER_NAMES = ('FusedClipSGD', 'FusedClipAdamW', 'GraphedStep', 'Trainer')


def __getattr__(name):
    """The training surface (``sqd.FusedClipAdamW`` ...), imported from ``trainer`` on first use."""
    if name in _TRAINER_NAMES:
        from . import trainer
        return getattr(trainer, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
