from .kitti_dataset import KITTIDataset  # noqa: F401
from .nuscenes_dataset import nuScenesDataset  # noqa: F401
from .synthetic import SyntheticTriplets  # noqa: F401
from .waymo_dataset import WaymoDataset  # noqa: F401
from .folder_dataset import FolderDataset  # noqa: F401
