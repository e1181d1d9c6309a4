"""predict.main in a process of its own, for tests/test_cloud_gpu.py: every run named in the job file over one folder of frames, with
predict_batch recording what it returned (as tests/test_predict_gpu.py records it).  predict.py sets the process up the way a
command-line tool does -- MIOpen's find mode and user database at import, the recorded GEMM solutions with the Trainer -- and that
set-up would reach every test file behind the caller's if it happened inside the test process.

    python cloud_predict_worker.py <job.json>      {"frames": dir, "out": dir, "runs": {name: [predict.py arguments]}}

Per run: <out>/<name>/ (predict.py's output), <out>/<name>_seen.npz ("<stem>/<key>" -> that frame's tensor, in the order seen) and
<out>/<name>_written.json (the paths predict.main returned)."""
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
    for name, extra in job["runs"].items():
        seen = {}

        def recording(opt, trainer, inputs, _seen=seen, **kwargs):
            res = inner(opt, trainer, inputs, **kwargs)
            for b, stem in enumerate(inputs["paths"]):
                for k, v in res.items():
                    _seen["{}/{}".format(stem, k)] = v[b].float().cpu().numpy()
            return res

        predict.predict_batch = recording
        torch.manual_seed(0)
        out = os.path.join(job["out"], name)
        written = predict.main([job["frames"]] + list(extra) + ["--log_dir", os.path.join(job["out"], "logs_" + name), "--out", out])
        np.savez(os.path.join(job["out"], name + "_seen.npz"), **seen)
        with open(os.path.join(job["out"], name + "_written.json"), "w") as fh:
            json.dump(written, fh)


if __name__ == "__main__":
    main(sys.argv[1])
