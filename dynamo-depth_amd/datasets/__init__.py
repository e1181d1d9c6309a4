from .kitti_dataset import KITTIDataset  # noqa: F401
from .nuscenes_dataset import nuScenesDataset  # noqa: F401
from .synthetic import SyntheticTriplets, WaymoDataset  # noqa: F401
