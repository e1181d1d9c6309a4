"""The nuScenes JSON tables that prepare_data/nuScenes.py walks, read without the devkit: token look-up and the two reverse indices
of the devkit's NuScenes class that the script uses (sample -> key-frame data by channel, sample -> annotations in table order).
No pandas, no map tables.  `category.index` is the field the panoptic / lidarseg package adds to category.json."""
import json
import os.path as osp

import numpy as np

TABLES = ("scene", "sample", "sample_data", "calibrated_sensor", "ego_pose", "sensor", "category", "attribute", "sample_annotation", "instance",
          "panoptic")


class Tables:
    def __init__(self, data_root, version="v1.0-trainval"):
        self.data_root, self.version = data_root, version
        for name in TABLES:
            path = osp.join(data_root, version, name + ".json")
            if not osp.exists(path):
                raise FileNotFoundError("nuScenes table {} is missing (the panoptic package provides panoptic.json)".format(path))
            with open(path, "r") as fh:
                setattr(self, name, json.load(fh))
        for c in self.category:
            if "index" not in c:
                raise KeyError("category.json of {} has no `index` field: install the category.json of the nuScenes-panoptic / "
                               "nuScenes-lidarseg package over it, as the devkit requires".format(osp.join(data_root, version)))
        self._by_token = {name: {r["token"]: r for r in getattr(self, name)} for name in TABLES if name != "panoptic"}
        self._by_token["panoptic"] = {r["sample_data_token"]: r for r in self.panoptic}        # looked up by the lidar's token, as the devkit does
        for s in self.sample:
            s["data"], s["anns"] = {}, []
        for sd in self.sample_data:
            sensor = self.get("sensor", self.get("calibrated_sensor", sd["calibrated_sensor_token"])["sensor_token"])
            sd["channel"] = sensor["channel"]
            if sd["is_key_frame"]:
                self.get("sample", sd["sample_token"])["data"][sensor["channel"]] = sd["token"]
        for ann in self.sample_annotation:
            ann["category_name"] = self.get("category", self.get("instance", ann["instance_token"])["category_token"])["name"]
            self.get("sample", ann["sample_token"])["anns"].append(ann["token"])

    def get(self, table, token):
        return self._by_token[table][token]

    def linked_list(self, first, table):
        """The records from `first` along `next`, with the reference's check of `prev`."""
        out = [first]
        while out[-1]["next"] != "":
            nxt = self.get(table, out[-1]["next"])
            assert nxt["prev"] == out[-1]["token"]
            out.append(nxt)
        return out


def read_scan(path):
    """A LIDAR_TOP .pcd.bin file: float32 (n, 5) [x, y, z, intensity, ring]; the first four columns, as the devkit keeps them."""
    return np.ascontiguousarray(np.fromfile(path, dtype=np.float32).reshape(-1, 5)[:, :4])


def read_panoptic(path):
    """A panoptic .npz file: the uint16 `data` array, one label (category * 1000 + instance) per point."""
    with np.load(path) as z:
        return z["data"].astype(np.uint16)
