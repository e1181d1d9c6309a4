"""Waymo loader over the reference's processed layout
<data_path>/<folder>/<cam>/{rgb/{cam.json,<img_type>/<frame:06>.jpg},depth/<frame:06>.npy,mask/<frame:06>.{npz,pickle}}
(reference datasets/waymo_dataset.py:9-120).  The motion mask is stored as per-object contour lists; the reference fills them with
cv2.drawContours, here hipops.contours does: in numpy on the host (get_mask), or on the device from the fixed-size records of
get_mask_contours."""
import json
import os
import pickle

import numpy as np
import PIL.Image as pil

from .base_dataset import BaseDataset

CATEGORIES = ("undefined", "ego_vehicle", "car", "truck", "bus", "other_vehicle", "bicycle", "motorcycle", "trailer", "pedestrian", "bicyclist",
              "motorcyclist", "bird", "ground_animal", "const_cone_pole", "pole", "pedestrian_stuff", "sign", "traffix_light", "building", "road",
              "lane_marker", "road_marker", "sidewalk", "vegetation", "sky", "ground", "dynamic", "static")
MOVING_SPEED = 1.0                  # m/s: an object with a box is `moving` (label 1) above it, `static` (2) otherwise; without a box 3


class WaymoDataset(BaseDataset):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.full_res_shape = (1920, 1280)
        self.categories = dict(enumerate(CATEGORIES))
        self.mask_caps = None                                   # (vertices, contours) per sample of the device records; None: hipops.contours' defaults
        # intrinsics normalised by the image size, one matrix per segment
        self.K = {}
        for folder in sorted({f.split()[0] for f in self.filenames}):
            with open(os.path.join(self._cam_dir(folder), "rgb", "cam.json"), "r") as fh:
                K = np.eye(4, dtype=np.float32)
                K[:3, :3] = np.array(json.load(fh)["intrinsic_mat"])
                self.K[folder] = K

    def _cam_dir(self, folder):
        return os.path.join(self.data_path, folder, self.cam_name)

    def get_intrinsic(self, folder):
        return self.K[folder]

    def get_gt_dim(self, folder, frame_index, side):
        return self.full_res_shape[1], self.full_res_shape[0]

    def get_timestep(self, folder, frame_index, offset):
        return 1                                                # the frames are evenly spaced

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

    def _mask_paths(self, folder, frame_index):
        stem = os.path.join(self._cam_dir(folder), "mask", "{:06d}".format(frame_index))
        return stem + ".npz", stem + ".pickle"

    def get_mask_objects(self, folder, frame_index, side):
        """(semantic mask (H, W) uint8, [(motion label, [contour (n, 2) [x, y], ...]), ...] in file order, name for messages); zeros
        and no objects when the frame has no annotation."""
        width, height = self.full_res_shape
        sem_path, mot_path = self._mask_paths(folder, frame_index)
        if not os.path.exists(sem_path):
            return np.zeros((height, width), dtype=np.uint8), [], sem_path
        sem = np.ascontiguousarray(np.load(sem_path)["semantic"].reshape(height, width), dtype=np.uint8)
        with open(mot_path, "rb") as fh:
            entries = pickle.load(fh)
        objects = []
        for obj in entries:
            if obj["box_label"] is None:
                label = 3                                       # unlabelled
            elif np.sqrt(np.sum(np.array(obj["speed"]) ** 2)) > MOVING_SPEED:
                label = 1                                       # in motion
            else:
                label = 2                                       # static
            objects.append((label, [np.asarray(c).reshape(-1, 2) for c in obj["mask"]]))
        return sem, objects, mot_path

    def get_mask(self, folder, frame_index, side, do_flip):
        """(semantic mask, motion mask) at full resolution, not flipped (as in the reference).  Motion: 1 = moving, 2 = static,
        3 = unlabelled object, 0 = background; the objects are painted in file order."""
        from hipops import contours
        sem, objects, name = self.get_mask_objects(folder, frame_index, side)
        return sem, contours.fill_host(objects, self.full_res_shape[1], self.full_res_shape[0], name)

    def get_mask_contours(self, folder, frame_index, side):
        """(semantic mask, vertices, contour records) for hipops.contours.fill_contours, or (semantic mask, motion mask) filled on the
        host for a frame whose contours exceed the fixed records."""
        from hipops import contours
        sem, objects, name = self.get_mask_objects(folder, frame_index, side)
        width, height = self.full_res_shape
        try:
            v_cap, c_cap = self.mask_caps or (contours.V_CAP, contours.C_CAP)
            return (sem,) + contours.pack(objects, height, width, name, v_cap, c_cap)
        except contours.OverCap:
            return sem, contours.fill_host(objects, height, width, name)
