"""The yardstick of the motion-segmentation tests, written out: the reference's scan (eval/motion_segmentation.py:52-95,118-140) --
F.interpolate to ground-truth size, `> thrds` broadcast to (T, H, W) per sample, its three sums, and the per-class false positives --
on the tensors' own device.  `expected_counts` turns the scan into the (2 + num_sem, T + 1) histogram layout of dd_motion_pr."""
import torch
import torch.nn.functional as F


def reference_thrds(num_thrd=150):
    eps = 1 / (num_thrd - 1)
    return torch.linspace(0 - eps, 1 - eps, num_thrd)


def upsample(pred, size):
    return F.interpolate(pred, size, mode="bilinear", align_corners=False)


def scan(pred, mot, sem, thrds, num_sem):
    """tp, p_sum (T,), g_sum, n_valid (scalars), fp_sem (num_sem, T), n_sem (num_sem,): int64 on the CPU; one sample at a time."""
    T = thrds.numel()
    up = upsample(pred, tuple(mot.shape[1:]))
    th = thrds.to(pred.device).reshape(T, 1, 1)
    tp, p_sum = torch.zeros(T, dtype=torch.int64), torch.zeros(T, dtype=torch.int64)
    fp_sem, n_sem = torch.zeros(num_sem, T, dtype=torch.int64), torch.zeros(num_sem, dtype=torch.int64)
    g_sum = n_valid = 0
    for b in range(pred.shape[0]):
        pm = up[b] > th                                        # (T, H, W)
        gm, vm = (mot[b] == 1)[None], (mot[b] != 3)[None]
        tp += torch.logical_and(gm, pm).sum((1, 2)).cpu()
        p_sum += (pm * vm).sum((1, 2)).cpu()
        g_sum += int(gm.sum())
        n_valid += int(vm.sum())
        for l in range(num_sem):
            cls = (vm & ~gm & (sem[b] == l)[None])
            fp_sem[l] += torch.logical_and(cls, pm).sum((1, 2)).cpu()
            n_sem[l] += int(cls.sum())
    return {"tp": tp, "p_sum": p_sum, "g_sum": g_sum, "n_valid": n_valid, "fp_sem": fp_sem, "n_sem": n_sem}


def hist_from_above(above, total):
    """above[k] = #{pixels exceeding threshold k} (non-increasing in k for an ascending table) -> the T + 1 bins by number of
    thresholds exceeded."""
    above = above.to(torch.int64)
    return torch.cat([torch.tensor([total], dtype=torch.int64) - above[:1], above[:-1] - above[1:], above[-1:]])


def expected_counts(pred, mot, sem, thrds, num_sem):
    s = scan(pred, mot, sem, thrds, num_sem)
    rows = [hist_from_above(s["tp"], s["g_sum"]), hist_from_above(s["p_sum"], s["n_valid"])]
    rows += [hist_from_above(s["fp_sem"][l], int(s["n_sem"][l])) for l in range(num_sem)]
    return torch.stack(rows)


def above_from_counts(counts):
    """[r, k] = sum over bins > k of row r."""
    return counts.cpu().flip(1).cumsum(1).flip(1)[:, 1:]


def dyadic_case(B, h, w, H, W, seed, sem_max=32):
    """pred: multiples of 1/256 in [0, 1] (at an integer scale factor every bilinear product is then exact in fp32, whatever the
    order or contraction of the operations); mot uniform in {0..3}; sem uniform in {0..sem_max-1}."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(0, 257, (B, 1, h, w), generator=g).float() / 256
    mot = torch.randint(0, 4, (B, H, W), generator=g, dtype=torch.uint8)
    sem = torch.randint(0, sem_max, (B, H, W), generator=g, dtype=torch.uint8)
    return pred, mot, sem


def near_threshold_counts(ref_up, thrds, tol=1e-6):
    """n_k = #{pixels : |ref_up - thr_k| <= tol} (T,), and the number of pixels within tol of ANY threshold."""
    flat = ref_up.reshape(-1)
    th = thrds.to(flat.device)
    n = torch.zeros(th.numel(), dtype=torch.int64)
    anyk = torch.zeros_like(flat, dtype=torch.bool)
    for k in range(th.numel()):
        close = (flat - th[k]).abs() <= tol
        n[k] = int(close.sum())
        anyk |= close
    return n, int(anyk.sum())


def assert_decision_masked(got_counts, pred, mot, thrds, max_share=1e-3, tol=1e-6):
    """|got - ref| <= n_k for tp, p_sum and g_sum at every threshold, n_k the pixels whose reference value lies within `tol` of
    threshold k (two fp32 evaluations of the same taps may differ by a few ulp under FMA contraction: 1e-6 covers that for values
    in [0, 1]); fails as vacuous when more than `max_share` of the pixels lie that close to any threshold."""
    ref = scan(pred, mot, None, thrds, 0)
    n, n_any = near_threshold_counts(upsample(pred, tuple(mot.shape[1:])), thrds, tol)
    share = n_any / mot.numel()
    above = above_from_counts(got_counts)
    got_g = int(got_counts[0].sum())
    worst = {name: int((g - r).abs().max()) for name, g, r in (("tp", above[0], ref["tp"]), ("p_sum", above[1], ref["p_sum"]))}
    print("decision-masked: {} pixels, {} within {:g} of a threshold (share {:.2e}), max n_k {}, worst |got - ref| {} g_sum {} vs {}".format(
        mot.numel(), n_any, tol, share, int(n.max()), worst, got_g, ref["g_sum"]))
    assert share <= max_share, "vacuous: {:.2e} of the pixels lie within {:g} of a threshold".format(share, tol)
    assert bool(((above[0] - ref["tp"]).abs() <= n).all()), ("tp", above[0] - ref["tp"], n)
    assert bool(((above[1] - ref["p_sum"]).abs() <= n).all()), ("p_sum", above[1] - ref["p_sum"], n)
    assert abs(got_g - ref["g_sum"]) <= int(n.min()), ("g_sum", got_g, ref["g_sum"])
