"""predict.main in a process of its own, for tests/test_tracks_gpu.py (tests/cloud_predict_worker.py says why a process of its own):
three runs over one folder of frames with predict_batch recording what it returned.

    python tracks_predict_worker.py <job.json>      {"frames": dir, "out": dir, "base": [predict.py arguments], "min_pixels": n}

Run `plain`: base + --save depth16.  The median of the motion mask of its first batch becomes the threshold (<out>/thresh.json) of the
two other runs -- an untrained network's mask lies in a narrow band somewhere in (0, 1), and the frames are to hold some but not all
foreground.  Run `objects`: base + --save depth16 objects; run `tracks`: base + --save depth16 objects tracks, both with
--object_motion_thresh <median> --object_min_pixels n.  All runs seed torch alike, so their networks are the same.  Per run:
<out>/<name>/, <out>/<name>_seen.npz ("<stem>/<key>" -> that frame's tensor) and <out>/<name>_written.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamo-depth_amd")]

import predict  # noqa: E402  (first: it prepares the environment before torch is imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(job_file):
    with open(job_file) as fh:
        job = json.load(fh)
    inner = predict.predict_batch
    first_masks = []

    def run(name, extra):
        seen = {}

        def recording(opt, trainer, inputs, **kwargs):
            res = inner(opt, trainer, inputs, **kwargs)
            if not seen:
                first_masks.append(res["motion_mask"].float().cpu().numpy())
            for b, stem in enumerate(inputs["paths"]):
                for k, v in res.items():
                    seen["{}/{}".format(stem, k)] = v[b].float().cpu().numpy()
            return res

        predict.predict_batch = recording
        torch.manual_seed(0)
        out = os.path.join(job["out"], name)
        written = predict.main([job["frames"]] + list(job["base"]) + list(extra) + ["--log_dir", os.path.join(job["out"], "logs_" + name), "--out", out])
        np.savez(os.path.join(job["out"], name + "_seen.npz"), **seen)
        with open(os.path.join(job["out"], name + "_written.json"), "w") as fh:
            json.dump(written, fh)

    run("plain", ["--save", "depth16"])
    thresh = float(np.float32(np.median(first_masks[0])))
    with open(os.path.join(job["out"], "thresh.json"), "w") as fh:
        json.dump(thresh, fh)
    objects = ["--object_motion_thresh", repr(thresh), "--object_min_pixels", str(job["min_pixels"])]
    run("objects", ["--save", "depth16", "objects"] + objects)
    run("tracks", ["--save", "depth16", "objects", "tracks"] + objects + list(job.get("tracks", [])))


if __name__ == "__main__":
    main(sys.argv[1])
