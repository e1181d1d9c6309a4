"""nuScenes loader over the reference's processed layout
<data_path>/<folder>/<cam>/{rgb/{cam.json,ts.json,<img_type>/<frame:06>.jpg},depth/<frame:06>.npy,mask/<frame:06>.npz}
(reference datasets/nuscenes_dataset.py:10-97).  The motion labels are per LiDAR point; the mask is their 5x5-pixel footprint."""
import json
import os

import numpy as np
import PIL.Image as pil

from .base_dataset import BaseDataset

MASK_CELL = 5                       # side of a LiDAR point's footprint in the motion mask, in full-resolution pixels
MEDIAN_TS = 100.0                   # the unit of ('ts', f): the median frame interval of the processed sequences


class nuScenesDataset(BaseDataset):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.full_res_shape = (1600, 900)
        # intrinsics normalised by the image size, one matrix per scene
        self.K = {}
        for folder in sorted({f.split()[0] for f in self.filenames}):
            with open(os.path.join(self._cam_dir(folder), "rgb", "cam.json"), "r") as fh:
                K = np.eye(4, dtype=np.float32)
                K[:3, :3] = np.array(json.load(fh)["intrinsic_mat"])
                self.K[folder] = K
        self._ts = {}

    def _cam_dir(self, folder):
        return os.path.join(self.data_path, folder, self.cam_name)

    def get_intrinsic(self, folder):
        return self.K[folder]

    def get_gt_dim(self, folder, frame_index, side):
        return self.full_res_shape[1], self.full_res_shape[0]

    def get_timestep(self, folder, frame_index, offset):
        """Time between frame_index and frame_index + offset in units of the median frame interval."""
        if folder not in self._ts:
            with open(os.path.join(self._cam_dir(folder), "rgb", "ts.json"), "r") as fh:
                self._ts[folder] = json.load(fh)
        low, high = min(frame_index, frame_index + offset), max(frame_index, frame_index + offset)
        return np.sum(self._ts[folder][low:high]) / MEDIAN_TS

    def get_img_path(self, folder, frame_index, side):
        return os.path.join(self._cam_dir(folder), "rgb", self.img_type, "{:06d}{}".format(frame_index, self.img_ext))

    def get_color(self, folder, frame_index, side, do_flip):
        img = self.loader(self.get_img_path(folder, frame_index, side))
        return img.transpose(pil.FLIP_LEFT_RIGHT) if do_flip else img

    def get_color_bytes(self, folder, frame_index, side):
        with open(self.get_img_path(folder, frame_index, side), "rb") as fh:
            return fh.read()

    def get_depth(self, folder, frame_index, side, do_flip):
        lidar = np.load(os.path.join(self._cam_dir(folder), "depth", "{:06d}.npy".format(frame_index)))     # (N,3) [col, row, z]
        if do_flip:
            lidar[:, 0] = self.full_res_shape[0] - lidar[:, 0]
        return lidar[:, [1, 0, 2]]                                                                          # [row, col, z]

    def get_mask(self, folder, frame_index, side, do_flip):
        """(semantic mask, motion mask) at full resolution.  nuScenes has no semantic image labels: all ones.  Motion: every LiDAR
        point labels the 5x5-pixel cell it falls in (1 = moving, 2 = static, 0 = background), cells without a point are 3 =
        unlabelled -- the reference scatters onto a 180x320 grid and resizes it by 5 with nearest neighbour, which at an exact
        integer factor replicates every cell."""
        width, height = self.full_res_shape
        path = os.path.join(self._cam_dir(folder), "mask", "{:06d}.npz".format(frame_index))
        if not os.path.exists(path):
            return np.zeros((height, width), dtype=np.uint8), np.full((height, width), 3, dtype=np.uint8)
        labels = np.load(path)["motion_label"]
        points = self.get_depth(folder, frame_index, side, False)
        rows = np.clip((points[:, 0] / MASK_CELL).astype(np.int64), 0, height // MASK_CELL - 1)
        cols = np.clip((points[:, 1] / MASK_CELL).astype(np.int64), 0, width // MASK_CELL - 1)
        grid = np.full((height // MASK_CELL, width // MASK_CELL), 3, dtype=np.uint8)
        for r, c, l in zip(rows.tolist(), cols.tolist(), labels.tolist()):                                 # in file order: the last point of a cell wins
            grid[r, c] = l
        mot = np.repeat(np.repeat(grid, MASK_CELL, axis=0), MASK_CELL, axis=1)
        return np.ones((height, width), dtype=np.uint8), mot
