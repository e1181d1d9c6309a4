"""Loss operators of Dynamo-Depth with the reference's Python signatures (tools.py:6-326), backed by the
HIP library instead of chains of ATen kernels.

This module is the drop-in operator boundary: BackprojectDepth, Project3D, SSIM,
GroundPlane, DepthMetrics, disp_to_depth, depth_to_disp, compute_smooth_loss, compute_errors, torch_and.
Every differentiable operator is a torch.autograd.Function over the C ABI (hipops.functions); tensors must
be on the GPU -- there is no CPU implementation of the loss path and none is silently substituted.
(DepthMetrics is evaluation bookkeeping on gathered LiDAR hits and stays in plain torch.)
MotionSegMetrics is the motion-mask evaluation of the reference's eval/motion_segmentation.py as an accumulating class;
DepthMetricsAccumulator and OdometryMetrics are the cross-batch bookkeeping of its eval/depth.py and eval/odometry.py, kept on the device.
"""
import numpy as np
import torch
import torch.nn as nn

from hipops import functions as HF
from hipops import lib as L


def disp_to_depth(disp, min_depth, max_depth):
    """Sigmoid disparity -> (scaled disparity, depth): 1/max + (1/min - 1/max)*disp (reference tools.py:291-298)."""
    return HF.DispToDepthFn.apply(disp, float(min_depth), float(max_depth))


def depth_to_disp(depth, min_depth, max_depth):
    """Inverse of disp_to_depth (reference tools.py:301-308)."""
    lo, hi = 1 / max_depth, 1 / min_depth
    return (1 / depth - lo) / (hi - lo)


def compute_smooth_loss(inp, img=None):
    """Edge-aware first-order smoothness of a (B,C,H,W) tensor (reference tools.py:311-326)."""
    return HF.SmoothLossFn.apply(inp, img, False)


class BackprojectDepth(nn.Module):
    """depth (B,1,h,w), inv_K (B,4,4) -> homogeneous points (B,4,h*w) (reference tools.py:167-197).
    `pix_coords` is kept as a buffer-like attribute because Trainer.get_ground_depth reads it."""

    def __init__(self, batch_size, height, width):
        super().__init__()
        self.batch_size, self.height, self.width = batch_size, height, width
        ys, xs = np.meshgrid(range(height), range(width), indexing="ij")
        pix = np.stack([xs.reshape(-1), ys.reshape(-1), np.ones(height * width)], 0).astype(np.float32)
        self.pix_coords = nn.Parameter(torch.from_numpy(pix).unsqueeze(0).repeat(batch_size, 1, 1), requires_grad=False)

    def forward(self, depth, inv_K):
        if depth.shape[-2:] != (self.height, self.width):
            raise ValueError("BackprojectDepth built for {}x{}, got {}".format(self.height, self.width, tuple(depth.shape[-2:])))
        return HF.BackprojectFn.apply(depth, inv_K)


class Project3D(nn.Module):
    """points (B,4,N), K, T|None -> (sampling grid (B,h,w,2) in [-1,1], ego motion (B,3,N)) (reference tools.py:200-224)."""

    def __init__(self, batch_size, height, width, eps=1e-7):
        super().__init__()
        self.batch_size, self.height, self.width, self.eps = batch_size, height, width, eps

    def forward(self, points, K, T):
        return HF.Project3DFn.apply(points, K, T, self.height, self.width, float(self.eps))


class SSIM(nn.Module):
    """clamp((1 - SSIM(x,y))/2, 0, 1) with 3x3 box statistics over reflection-padded images (reference tools.py:227-257)."""

    def __init__(self):
        super().__init__()
        self.C1, self.C2 = 0.01 ** 2, 0.03 ** 2

    def forward(self, x, y):
        return HF.SSIMFn.apply(x, y)


class GroundPlane(nn.Module):
    """RANSAC ground plane y = w1*x + w2*z + w3 on the bottom `g_prior` of a point map (reference tools.py:76-164).
    forward(points (B,3,H,W)) -> (distance (B,1,H,W), plane (B,3,1)), both detached.  The candidate indices come
    from the global NumPy RNG like the reference's (tools.py:125-127) unless `rand_idx` is injected."""

    def __init__(self, num_points_per_it=5, max_it=25, tol=0.1, g_prior=0.5, vertical_axis=1):
        super().__init__()
        if vertical_axis != 1:
            raise NotImplementedError("the HIP ground-plane kernels assume the camera convention y = down (vertical_axis=1)")
        self.num_points_per_it, self.max_it, self.tol, self.g_prior, self.vertical_axis = num_points_per_it, max_it, tol, g_prior, vertical_axis

    def draw_indices(self, B, H, W):
        n_ground = int(self.g_prior * H) * W
        total = self.num_points_per_it * self.max_it
        return np.stack([np.random.choice(np.arange(n_ground), total, replace=True) for _ in range(B)])

    def forward(self, points, rand_idx=None):
        import ctypes as C
        from hipops import abi
        pts = HF._dev(points.detach(), "points")
        B, _, H, W = pts.shape
        if rand_idx is None:
            rand_idx = self.draw_indices(B, H, W)
        ridx = torch.as_tensor(np.asarray(rand_idx), dtype=torch.int32).to(pts.device).contiguous()
        lib = L.load()
        dist = torch.empty(B, 1, H, W, dtype=torch.float32, device=pts.device)
        plane = torch.empty(B, 3, dtype=torch.float32, device=pts.device)
        ws = HF._ws(lib.dd_ground_workspace_bytes(B, H, W, self.max_it), pts.device)
        L.check(lib.dd_ground_plane(abi.ptr(pts), abi.ptr(ridx), B, H, W, self.num_points_per_it, self.max_it, float(self.tol),
                                    float(self.g_prior), abi.ptr(dist), abi.ptr(plane), abi.ptr(ws), L.current_stream()), "dd_ground_plane")
        return dist, plane.unsqueeze(-1)


def torch_and(*args):
    out = args[0]
    for a in args:
        assert out.size() == a.size(), "Sizes must match: [{}]".format(", ".join(str(x.size()) for x in args))
        out = torch.logical_and(out, a)
    return out


def compute_errors(gt, pred):
    """abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 (Eigen et al.), reference tools.py:269-288."""
    ratio = torch.max(gt / pred, pred / gt)
    a1, a2, a3 = [(ratio < 1.25 ** k).float().mean() for k in (1, 2, 3)]
    rmse = torch.sqrt(((gt - pred) ** 2).mean())
    rmse_log = torch.sqrt(((torch.log(gt) - torch.log(pred)) ** 2).mean())
    abs_rel = torch.mean(torch.abs(gt - pred) / gt)
    sq_rel = torch.mean((gt - pred) ** 2 / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3


class MotionSegMetrics:
    """Precision / recall / F1 of the motion mask over `num_thrd` thresholds at ground-truth resolution, and the per-class tally of
    false positives (reference eval/motion_segmentation.py:52-95,118-140), as ONE integer histogram: a pixel's bin is the number
    of thresholds its up-sampled prediction exceeds, so tp / fp / fn of every threshold -- and the false positives of every class
    at any threshold -- are suffix sums of `counts` (2 + num_sem, num_thrd + 1): row 0 = moving pixels (mot == 1), row 1 =
    labelled pixels (mot != 3), row 2+l = labelled non-moving pixels of class l.  No (B, T, H, W) scan, no stored prediction, no
    second pass.  The reference accumulates its sums in float32, inexact above 2**24 pixels; these are exact integers.

    update() on CUDA tensors is one dd_motion_pr launch on the current stream (no host sync); CPU tensors take the same
    formulation in torch.  `thrds` (optional) replaces the reference's table with any ascending 1-D table of num_thrd entries."""

    def __init__(self, num_thrd=150, num_sem=0, thrds=None):
        if not 1 <= num_thrd <= 256 or not 0 <= num_sem <= 32:
            raise ValueError("MotionSegMetrics: 1 <= num_thrd <= 256 and 0 <= num_sem <= 32, got {} and {}".format(num_thrd, num_sem))
        self.num_thrd, self.num_sem = int(num_thrd), int(num_sem)
        if thrds is None:
            eps = 1 / (num_thrd - 1)                             # as the reference builds it (eval/motion_segmentation.py:52-53)
            thrds = torch.linspace(0 - eps, 1 - eps, num_thrd)
        self.thrds = torch.as_tensor(thrds, dtype=torch.float32).reshape(-1).contiguous()
        if self.thrds.numel() != self.num_thrd or bool((self.thrds[1:] < self.thrds[:-1]).any()):
            raise ValueError("MotionSegMetrics: thrds must hold num_thrd ascending values")
        self.counts = None

    def reset(self):
        self.counts = None

    def update(self, pred_mask, mot_mask, sem_mask=None):
        """pred_mask (B,1,h,w) float; mot_mask, sem_mask (B,H,W) uint8 on the same device."""
        if pred_mask.dim() != 4 or pred_mask.shape[1] != 1 or mot_mask.dim() != 3 or mot_mask.shape[0] != pred_mask.shape[0]:
            raise ValueError("MotionSegMetrics.update: pred_mask (B,1,h,w) and mot_mask (B,H,W), got {} and {}".format(
                tuple(pred_mask.shape), tuple(mot_mask.shape)))
        if self.num_sem > 0 and (sem_mask is None or sem_mask.shape != mot_mask.shape):
            raise ValueError("MotionSegMetrics.update: num_sem > 0 needs a sem_mask of mot_mask's shape")
        dev = pred_mask.device
        pred = pred_mask.detach().to(torch.float32).contiguous()
        mot = mot_mask.to(dev, torch.uint8).contiguous()
        sem = sem_mask.to(dev, torch.uint8).contiguous() if self.num_sem > 0 else None
        if self.counts is None:
            self.counts = torch.zeros((2 + self.num_sem, self.num_thrd + 1), dtype=torch.int64, device=dev)    # the kernel's uint64, same bits
        self.thrds = self.thrds.to(dev)
        if pred.is_cuda:
            from hipops import abi
            B, _, h, w = pred.shape
            L.check(L.load().dd_motion_pr(abi.ptr(pred), B, h, w, abi.ptr(mot), abi.ptr(sem), mot.shape[1], mot.shape[2], abi.ptr(self.thrds),
                                          self.num_thrd, self.num_sem, abi.ptr(self.counts), L.current_stream()), "dd_motion_pr")
        else:
            self.counts += self._counts_torch(pred, mot, sem)

    def _counts_torch(self, pred, mot, sem):
        nb = self.num_thrd + 1
        up = nn.functional.interpolate(pred, tuple(mot.shape[1:]), mode="bilinear", align_corners=False)[:, 0]
        bins = torch.searchsorted(self.thrds, up.contiguous(), right=False)        # #{k : thrds[k] < value}
        bins = torch.where(torch.isnan(up), torch.zeros_like(bins), bins)          # a NaN exceeds no threshold
        rows = [torch.bincount(bins[mot == 1], minlength=nb), torch.bincount(bins[mot != 3], minlength=nb)]
        rest = (mot != 1) & (mot != 3)
        rows += [torch.bincount(bins[rest & (sem == l)], minlength=nb) for l in range(self.num_sem)]
        return torch.stack(rows)

    def compute(self):
        if self.counts is None:
            raise RuntimeError("MotionSegMetrics.compute() before any update()")
        counts = self.counts.cpu()
        above = counts.flip(1).cumsum(1).flip(1)[:, 1:]                             # [r, k] = sum over bins > k of row r
        tp, p_sum = above[0], above[1]
        fp, fn = p_sum - tp, counts[0].sum() - tp
        tpd, fpd, fnd = tp.double(), fp.double(), fn.double()
        precision = tpd / (tpd + fpd + 1e-10)
        recall = tpd / (tpd + fnd + 1e-10)
        f1 = 2 * (precision * recall) / (precision + recall + 1e-10)
        best = int(torch.argmax(f1))
        out = {"tp": tp, "fp": fp, "fn": fn, "precision": precision.float(), "recall": recall.float(), "f1": f1.float(),
               "thrds": self.thrds.cpu(), "best_thrd_idx": best}
        if self.num_sem > 0:
            per_class = above[2:, best].tolist()
            tally = {l: c for l, c in enumerate(per_class) if c > 0}                # the classes that occur, as np.unique lists them
            tally["total"] = int(sum(per_class))
            out["fp_tally"] = tally
        return out


class DepthMetrics(nn.Module):
    """Sparse-LiDAR depth metrics with per-image median scaling (reference tools.py:6-73)."""

    def __init__(self, img_bound, min_depth, max_depth):
        super().__init__()
        self.depth_metric_names = ["de:abs_rel", "de:sq_rel", "de:rms", "de:log_rms", "da:a1", "da:a2", "da:a3"]
        self.img_bound, self.min_depth, self.max_depth = img_bound, min_depth, max_depth

    def forward(self, inputs, outputs, mask=None):
        disp_pred = outputs[("disp_scaled", 0, 0)]
        names = self.depth_metric_names
        if mask is None and disp_pred.is_cuda:
            return dict(zip(names, self.device_metrics(inputs, disp_pred)[1].unbind(0)))
        if mask is not None and disp_pred.is_cuda and mask.dim() == 3 and not mask.is_floating_point() and int(mask.max()) < 256 and int(mask.min()) >= 0:
            return self.device_metrics_masked(inputs, disp_pred, mask)
        return self._forward_torch(inputs, outputs, mask)

    def device_metrics_masked(self, inputs, disp_pred, mask):
        """The mask branch (reference tools.py:23-25,58-72) on the device: per-label errors of every sample in the same launch
        as the unmasked metrics; the host only builds the dict (one transfer for the label set, one for the totals)."""
        import ctypes as C
        names = self.depth_metric_names
        B, _, H, W = disp_pred.shape
        disp = disp_pred.detach().to(torch.float32).contiguous()
        lidar = inputs["depth_gt"].to(disp.device, torch.float32).contiguous()
        valid = inputs["depth_valid"].to(disp.device, torch.float32).contiguous()
        dims = inputs["gt_dim"].to(disp.device, torch.int32).contiguous()
        m8 = mask.to(disp.device, torch.uint8).contiguous()
        M = lidar.shape[1]
        lib = L.load()
        per = torch.empty((B, 8), dtype=torch.float32, device=disp.device)
        mean = torch.empty(7, dtype=torch.float32, device=disp.device)
        per_label = torch.empty((B, 256, 8), dtype=torch.float32, device=disp.device)
        nbytes = lib.dd_depth_metrics_masked_workspace_bytes(B, M)
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=disp.device)
        bound = (C.c_double * 4)(*[float(v) for v in self.img_bound])
        L.check(lib.dd_depth_metrics_masked(disp.data_ptr(), B, H, W, lidar.data_ptr(), valid.data_ptr(), M, dims.data_ptr(), bound,
                                            float(self.min_depth), float(self.max_depth), m8.data_ptr(), m8.shape[1], m8.shape[2], per.data_ptr(),
                                            mean.data_ptr(), per_label.data_ptr(), ws.data_ptr(), nbytes, L.current_stream()), "dd_depth_metrics_masked")
        metrics = dict(zip(names, mean.unbind(0)))
        labels = [int(l) for l in torch.unique(m8).tolist()]
        cnt = per_label[:, :, 7]                                                     # (B,256)
        weighted = (per_label[:, :, :7].double() * cnt.double().unsqueeze(-1)).sum(0).tolist()     # sum_b err * cnt, as the reference accumulates
        total = cnt.double().sum(0).tolist()
        for i, m in enumerate(names):
            metrics["{}_mask".format(m)] = {l: [weighted[l][i], int(total[l])] for l in labels}
        return metrics

    def device_metrics(self, inputs, disp_pred):
        """(per_sample (B,8), mean (7,)) from dd_depth_metrics: one workgroup per sample, exact medians, no host sync
        (the per-sample loop with .item() syncs of the reference, tools.py:27-66, in one launch)."""
        import ctypes as C
        B, _, H, W = disp_pred.shape
        disp = disp_pred.detach().to(torch.float32).contiguous()
        lidar = inputs["depth_gt"].to(disp.device, torch.float32).contiguous()
        valid = inputs["depth_valid"].to(disp.device, torch.float32).contiguous()
        dims = inputs["gt_dim"].to(disp.device, torch.int32).contiguous()
        M = lidar.shape[1]
        lib = L.load()
        per = torch.empty((B, 8), dtype=torch.float32, device=disp.device)
        mean = torch.empty(7, dtype=torch.float32, device=disp.device)
        nbytes = lib.dd_depth_metrics_workspace_bytes(B, M)
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=disp.device)
        bound = (C.c_double * 4)(*[float(v) for v in self.img_bound])
        L.check(lib.dd_depth_metrics(disp.data_ptr(), B, H, W, lidar.data_ptr(), valid.data_ptr(), M, dims.data_ptr(), bound,
                                     float(self.min_depth), float(self.max_depth), per.data_ptr(), mean.data_ptr(), ws.data_ptr(), nbytes,
                                     L.current_stream()), "dd_depth_metrics")
        return per, mean

    def _forward_torch(self, inputs, outputs, mask=None):
        disp_pred = outputs[("disp_scaled", 0, 0)]
        names = self.depth_metric_names
        metrics = {m: 0 for m in names}
        labels = []
        if mask is not None:
            labels = [l.item() for l in torch.unique(mask)]
            metrics.update({"{}_mask".format(m): {l: [0, 0] for l in labels} for m in names})
        for bi in range(disp_pred.size(0)):
            lidar, valid = inputs["depth_gt"][bi], inputs["depth_valid"][bi]
            gh, gw = inputs["gt_dim"][bi][0].item(), inputs["gt_dim"][bi][1].item()
            top, bottom = int(self.img_bound[0] * gh), int(self.img_bound[1] * gh)
            left, right = int(self.img_bound[2] * gw), int(self.img_bound[3] * gw)
            keep = torch_and(valid, lidar[:, 0] >= top, lidar[:, 0] < bottom, lidar[:, 1] >= left, lidar[:, 1] < right,
                             lidar[:, 2] > self.min_depth, lidar[:, 2] < self.max_depth)
            rows, cols = lidar[:, 0][keep].long(), lidar[:, 1][keep].long()
            full = 1 / nn.functional.interpolate(disp_pred[bi][None], (gh, gw), mode="bilinear", align_corners=False).squeeze()
            gt, pd = lidar[:, 2][keep], full[rows, cols]
            pd = torch.clamp(pd * (torch.median(gt) / torch.median(pd)), self.min_depth, self.max_depth)
            errs = compute_errors(gt, pd)
            for i, m in enumerate(names):
                metrics[m] += errs[i]
            if mask is not None:
                at = mask[bi][rows, cols]
                for l in labels:
                    pick = at == l
                    cnt = int(pick.sum())
                    if cnt == 0:
                        continue
                    e2 = compute_errors(gt[pick], pd[pick])
                    for i, m in enumerate(names):
                        metrics["{}_mask".format(m)][l][0] += e2[i].item() * cnt
                        metrics["{}_mask".format(m)][l][1] += cnt
        for m in names:
            metrics[m] = metrics[m] / disp_pred.size(0)
        return metrics


class DepthMetricsAccumulator:
    """DepthMetrics over a whole evaluation with the running totals on the device (the reference's eval/depth.py pulls seven scalars
    to the host per batch; DepthMetrics' mask branch adds a torch.unique over the mask and two transfers).  update() is two launches on
    the current stream -- dd_depth_metrics[_masked], then dd_depth_metrics_accumulate -- and returns nothing; compute() makes the one
    transfer.  Every total is summed by one thread in batch order, so the result does not depend on the batch size (a ragged last
    batch included).  GPU only: there is no torch fallback here."""

    def __init__(self, img_bound, min_depth, max_depth):
        import ctypes as C
        self.depth_metric_names = ["de:abs_rel", "de:sq_rel", "de:rms", "de:log_rms", "da:a1", "da:a2", "da:a3"]
        self.img_bound, self.min_depth, self.max_depth = img_bound, float(min_depth), float(max_depth)
        self._bound = (C.c_double * 4)(*[float(v) for v in img_bound])
        self.totals = self.label_totals = None
        self._buf = None            # (device, B, M, masked) -> per_sample, mean, per_label, workspace

    def reset(self):
        self.totals = self.label_totals = None

    def _buffers(self, dev, B, M, masked):
        lib = L.load()
        b = self._buf
        if b is None or b["dev"] != dev or b["B"] < B or b["M"] < M or (masked and b["per_label"] is None):
            cap_b, cap_m = max(B, b["B"] if b else 0), max(M, b["M"] if b else 0)
            masked = masked or bool(b and b["per_label"] is not None)
            nbytes = int(lib.dd_depth_metrics_masked_workspace_bytes(cap_b, cap_m))          # the larger of the two workspaces
            b = self._buf = {"dev": dev, "B": cap_b, "M": cap_m, "ws_bytes": nbytes,
                             "per_sample": torch.empty((cap_b, 8), dtype=torch.float32, device=dev),
                             "mean": torch.empty(7, dtype=torch.float32, device=dev),
                             "per_label": torch.empty((cap_b, 256, 8), dtype=torch.float32, device=dev) if masked else None,
                             "ws": HF._ws(nbytes, dev)}
        return b

    def update(self, inputs, disp_scaled, mask=None):
        """inputs: the loader's depth_gt (B,M,3), depth_valid (B,M), gt_dim (B,2); disp_scaled (B,1,H,W) = outputs['disp_scaled',0,0];
        mask (B,h,w) integer labels below 256 in ground-truth pixels, or None."""
        from hipops import abi
        lib = L.load()
        disp = HF._dev(disp_scaled.detach(), "disp_scaled")
        dev = disp.device
        B, _, H, W = disp.shape
        lidar = inputs["depth_gt"].to(dev, torch.float32).contiguous()
        valid = inputs["depth_valid"].to(dev, torch.float32).contiguous()
        dims = inputs["gt_dim"].to(dev, torch.int32).contiguous()
        M = lidar.shape[1]
        masked = mask is not None
        if masked and (mask.dim() != 3 or mask.shape[0] != B or mask.is_floating_point()):
            raise ValueError("DepthMetricsAccumulator.update: mask must be (B,h,w) integer labels, got {} {}".format(tuple(mask.shape), mask.dtype))
        if self.totals is None:
            self.totals = torch.zeros(9, dtype=torch.float64, device=dev)
        if masked and self.label_totals is None:
            self.label_totals = torch.zeros((256, 8), dtype=torch.float64, device=dev)
        b = self._buffers(dev, B, M, masked)
        stream = L.current_stream()
        if masked:
            m8 = mask.to(dev, torch.uint8).contiguous()
            L.check(lib.dd_depth_metrics_masked(abi.ptr(disp), B, H, W, abi.ptr(lidar), abi.ptr(valid), M, abi.ptr(dims), self._bound, self.min_depth,
                                                self.max_depth, abi.ptr(m8), m8.shape[1], m8.shape[2], abi.ptr(b["per_sample"]), abi.ptr(b["mean"]),
                                                abi.ptr(b["per_label"]), abi.ptr(b["ws"]), b["ws_bytes"], stream), "dd_depth_metrics_masked")
        else:
            L.check(lib.dd_depth_metrics(abi.ptr(disp), B, H, W, abi.ptr(lidar), abi.ptr(valid), M, abi.ptr(dims), self._bound, self.min_depth,
                                         self.max_depth, abi.ptr(b["per_sample"]), abi.ptr(b["mean"]), abi.ptr(b["ws"]), b["ws_bytes"], stream),
                    "dd_depth_metrics")
        L.check(lib.dd_depth_metrics_accumulate(abi.ptr(b["per_sample"]), abi.ptr(b["per_label"]) if masked else None, B, abi.ptr(self.totals),
                                                abi.ptr(self.label_totals) if masked else None, stream), "dd_depth_metrics_accumulate")

    def compute(self):
        if self.totals is None:
            raise RuntimeError("DepthMetricsAccumulator.compute() before any update()")
        names = self.depth_metric_names
        both = torch.cat([self.totals] + ([self.label_totals.reshape(-1)] if self.label_totals is not None else [])).cpu().numpy()      # the one transfer
        totals = both[:9]
        with np.errstate(invalid="ignore", divide="ignore"):
            out = {"overall": {m: float(totals[j] / totals[7]) for j, m in enumerate(names)}, "num": int(totals[7]), "skipped": int(totals[8])}
        if self.label_totals is not None:
            lt = both[9:].reshape(256, 8)
            out["by_label"] = {l: {m: float(lt[l, j] / lt[l, 7]) for j, m in enumerate(names)} for l in range(256) if lt[l, 7] > 0}
            out["label_counts"] = {l: int(lt[l, 7]) for l in range(256) if lt[l, 7] > 0}
        return out


class OdometryMetrics:
    """Absolute trajectory error and ground-truth speed over `track_length`-frame snippets (reference eval/odometry.py:19-41,70-96), one
    dd_odom_snippets launch per segment into a growing device buffer; nothing returns to the host before compute().  A segment of N frame
    pairs yields S = snippet_count(N) snippets, the last of them one point shorter than the others -- the reference's behaviour."""

    def __init__(self, track_length=5):
        if not 2 <= int(track_length) <= 16:
            raise ValueError("OdometryMetrics: 2 <= track_length <= 16, got {}".format(track_length))
        self.track_length = int(track_length)
        self.values = None          # (2, capacity) float64 on the device: ates, speeds
        self.used = 0
        self.segments = []          # (offset, S) per add_segment

    def snippet_count(self, N):
        """S of a segment with N frame pairs (dd_odom_snippet_count restated; -1 for N < 1)."""
        return -1 if N < 1 else max(0, min(N, N - self.track_length + 3))

    def reset(self):
        self.values, self.used, self.segments = None, 0, []

    def add_segment(self, pred_T, gt_global):
        """pred_T (N,4,4) fp32 on the device; gt_global (N+1, 3 or 4, 4) float64 (numpy or tensor), uploaded once."""
        from hipops import abi
        lib = L.load()
        pred = HF._dev(pred_T.detach(), "pred_T")
        if pred.dim() != 3 or tuple(pred.shape[1:]) != (4, 4) or pred.shape[0] < 1:
            raise ValueError("OdometryMetrics.add_segment: pred_T must be (N,4,4) with N >= 1, got {}".format(tuple(pred.shape)))
        N = pred.shape[0]
        gt = torch.as_tensor(gt_global, dtype=torch.float64)
        if gt.dim() != 3 or gt.shape[0] != N + 1 or gt.shape[1] not in (3, 4) or gt.shape[2] != 4:
            raise ValueError("OdometryMetrics.add_segment: gt_global must be (N+1, 3 or 4, 4) for N = {}, got {}".format(N, tuple(gt.shape)))
        if gt.shape[1] == 3:
            last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=gt.device).expand(N + 1, 1, 4)
            gt = torch.cat((gt, last), 1)
        gt = gt.to(pred.device).contiguous()
        S = int(lib.dd_odom_snippet_count(N, self.track_length))
        if self.values is None or self.used + S > self.values.shape[1]:
            grown = torch.zeros((2, max(2 * (self.used + S), 1024)), dtype=torch.float64, device=pred.device)
            if self.values is not None:
                grown[:, :self.used] = self.values[:, :self.used]
            self.values = grown
        ate, speed = self.values[0, self.used:], self.values[1, self.used:]
        L.check(lib.dd_odom_snippets(abi.ptr(pred), abi.ptr(gt), N, self.track_length, abi.ptr(ate) if S else None, abi.ptr(speed) if S else None,
                                     L.current_stream()), "dd_odom_snippets")
        self.segments.append((self.used, S))
        self.used += S

    def compute(self):
        """{'ates', 'speeds': float64 numpy arrays over all snippets, 'segments': [(ates, speeds) slice per add_segment]}: one transfer."""
        if self.values is None:
            raise RuntimeError("OdometryMetrics.compute() before any add_segment()")
        both = self.values[:, :self.used].cpu().numpy()
        ates, speeds = both[0].copy(), both[1].copy()
        return {"ates": ates, "speeds": speeds, "segments": [(ates[o:o + s], speeds[o:o + s]) for o, s in self.segments]}
