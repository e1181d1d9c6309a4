"""A plain folder of frames (predict.py): every .jpg / .jpeg / .png file of one directory, sorted by name.  No depth, no masks, no
split list -- the reference's demo notebook reads its few frames with PIL one by one; here the folder is a BaseDataset, so baseline
JPEGs are decoded and resized on the device like any training frame and everything else takes the host path.

The sample line is "<dir> <index>", <index> the frame's position in the sorted list (`sample_lines`); frame offsets (--motion reads
the triplet i-1, i, i+1) are positions in that list too.  With path=True the item's 'paths' is the file's stem."""
import os

import numpy as np
import PIL.Image as pil

from .base_dataset import BaseDataset

EXTENSIONS = (".jpg", ".jpeg", ".png")
KITTI_K = ((0.58, 0, 0.5, 0), (0, 1.92, 0.5, 0), (0, 0, 1, 0), (0, 0, 0, 1))      # datasets/kitti_dataset.py


def list_frames(frames_dir):
    """The frame files of a directory, sorted by name."""
    return sorted(f for f in os.listdir(frames_dir) if f.lower().endswith(EXTENSIONS) and os.path.isfile(os.path.join(frames_dir, f)))


def sample_lines(frames_dir, indices):
    if len(str(frames_dir).split()) != 1:
        raise ValueError("a sample line is '<dir> <index>': the directory's path must not hold white space ({!r})".format(frames_dir))
    return ["{} {}".format(frames_dir, int(i)) for i in indices]


class FolderDataset(BaseDataset):
    def __init__(self, data_path, filenames=None, *args, intrinsics=None, **kwargs):
        """filenames None: one sample per frame.  intrinsics: (fx, fy, cx, cy) in pixels of the first frame, None for KITTI's."""
        self.frames = list_frames(data_path)
        if not self.frames:
            raise FileNotFoundError("no {} file in {}".format(" / ".join(EXTENSIONS), data_path))
        if filenames is None:
            filenames = sample_lines(data_path, range(len(self.frames)))
        kwargs.setdefault("img_ext", ".jpg")            # lets BaseDataset probe the device decoder; every file is looked at on its own
        kwargs["load_depth"] = kwargs["load_mask"] = False
        super().__init__(data_path, filenames, *args, **kwargs)
        self._sizes = {}
        self.K = np.array(KITTI_K, dtype=np.float32)
        if intrinsics is not None:
            fx, fy, cx, cy = (float(v) for v in intrinsics)
            gh, gw = self.get_gt_dim(None, 0, None)
            self.K[0, 0], self.K[0, 2], self.K[1, 1], self.K[1, 2] = fx / gw, cx / gw, fy / gh, cy / gh

    def get_img_path(self, folder, frame_index, side=None):
        if not 0 <= frame_index < len(self.frames):
            raise IndexError("frame {} of a folder of {}".format(frame_index, len(self.frames)))
        return os.path.join(self.data_path, self.frames[frame_index])

    def stem(self, frame_index):
        return os.path.splitext(self.frames[frame_index])[0]

    def get_color(self, folder, frame_index, side, do_flip):
        img = self.loader(self.get_img_path(folder, frame_index))
        return img.transpose(pil.FLIP_LEFT_RIGHT) if do_flip else img

    def get_color_bytes(self, folder, frame_index, side):
        with open(self.get_img_path(folder, frame_index), "rb") as fh:
            return fh.read()

    def get_intrinsic(self, folder):
        return self.K

    def get_gt_dim(self, folder, frame_index, side):
        if frame_index not in self._sizes:
            with pil.open(self.get_img_path(folder, frame_index)) as img:       # reads the header only
                self._sizes[frame_index] = (img.height, img.width)
        return self._sizes[frame_index]

    def __getitem__(self, index):
        item = super().__getitem__(index)
        _, frame, _ = self._sample_parts(index)
        import torch
        item["gt_dim"] = torch.tensor(self.get_gt_dim(None, frame, None)).type(torch.int)       # the sample's own frame, not its last neighbour
        if self.give_path:
            item["paths"] = self.stem(frame)
        return item
