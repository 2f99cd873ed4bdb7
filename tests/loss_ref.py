"""fp64 reference, exact-regime generators, case table and error bounds for the loss kernels of structuredetector_amd/csrc/sd_loss.hip
(k_loss_hm_partial, k_loss_finalize, k_loss_finalize_per_image, k_loss_bwd_dense, k_loss_bwd_scatter) and the fp64 reference of
k_render_targets (sd_encode.hip).  Plain numpy / torch-CPU: nothing here touches the GPU or the library.

Two input regimes (see docs/DESIGN_LOG.md, "Loss and target kernels: exact sums and fp64 bounds per branch"):

* exact: heatmap logits 0 (the sigmoid is exactly 0.5), heatmap targets from {0, 1/4, 1/2, 3/4, 1}, dyadic regression values and
  power-of-two loss weights.  Every term is a multiple of 1/16, every partial sum is exact in fp32 in any order, every product is
  exact so that an fma and a mul + add agree: the kernels must equal the restated values bit for bit after the final float cast.
* random: logits uniform in [-4, 4], targets in [0, 1) with exact 1.0 peaks and nextafter(1, 0) neighbours, saturated logits planted
  at |x| in {14.5, 20, 90} (never with 13 < |x| < 14.5, where the clamp's pass decision hangs on one ulp of expf) -> the kernels
  stay within BOUNDS of the fp64 reference.

BOUNDS are measured, not guessed: 16 x the largest deviation of the fp32 CPU oracle (oracle.sdnet_oracle.loss, torch fp32 with
autograd) from this fp64 reference over case_table() x {mse, focal}, with a floor of 4 * 2^-24 where the oracle does not deviate.
The factor covers the device's expf / logf (a few ulp where libm is at most 1 ulp) and the different summation tree.  Quantity
classes: "value" = the largest relative error of [total, hm, offset, embedding]; one class per channel group = max |got - ref| over
the group divided by the group's own max |ref|; "positives" = the t == 1 cells alone, divided by their own max |ref|.  Saturated
cells are left out of the toleranced classes (their gradient is asserted to be exactly 0); nothing else is.

Measured deviations of the fp32 oracle (tests/test_loss_ref_cpu.py::test_oracle_deviation_sets_the_bounds prints and asserts them):

    fn     value     anchor_hm  part_hm   offsets   embeddings  positives
    mse    1.40e-07  5.32e-07   5.24e-07  5.30e-08  4.37e-08    3.91e-07
    focal  4.59e-07  3.10e-07   3.03e-07  5.30e-08  4.37e-08    6.31e-07
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
CLAMP_LO = float(np.float32(1e-6))
CLAMP_HI = float(np.float32(1.0 - 1e-6))
LOSS_CHUNK = 4096                     # elements of one plane behind one block of k_loss_hm_partial / k_loss_bwd_dense
BLOCK_PASS = 1024                     # elements one pass of the 256 threads covers (one float4 each)
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
SATURATED = (14.5, -14.5, 20.0, -20.0, 90.0, -90.0)
SAT_SHARE_CAP = 0.01
DEFAULT_WEIGHTS = (1.0, 0.001, 0.001)
EXACT_WEIGHTS = (1.0, 0.5, 0.25)      # powers of two: go * w, w * x stay exact
GROUPS = ("anchor_hm", "part_hm", "offsets", "embeddings")
FLOOR = 4 * U

# 16 x the measured oracle deviation (module docstring), rounded up to two digits; FLOOR where the product is smaller
BOUNDS = {
    "mse": {"value": 2.3e-6, "anchor_hm": 8.6e-6, "part_hm": 8.4e-6, "offsets": 8.5e-7, "embeddings": 7.0e-7, "positives": 6.3e-6},
    "focal": {"value": 7.4e-6, "anchor_hm": 5.0e-6, "part_hm": 4.9e-6, "offsets": 8.5e-7, "embeddings": 7.0e-7, "positives": 1.1e-5},
}

# (h, w) -> the chunk case of k_loss_hm_partial it is the smallest plane for
SHAPES = {
    "one_float4": (1, 4),
    "idle_threads_384": (16, 24),
    "exactly_one_pass_1024": (32, 32),
    "two_chunks_tail_of_4": (41, 100),
    "whole_chunks_8192": (64, 128),
    "tail_chunk_of_4092": (89, 92),
}
PEAKS = ("both", "anchor", "part", "none")


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    return float(np.float32(v))


def chunk_plan(hw):
    """How k_loss_hm_partial walks a plane of hw elements: chunks, the length of the last one, its passes and its idle threads."""
    chunks = cdiv(hw, LOSS_CHUNK)
    last = hw - (chunks - 1) * LOSS_CHUNK
    return SimpleNamespace(chunks=chunks, last=last, passes=cdiv(last, BLOCK_PASS), live_last_pass=cdiv(last - (cdiv(last, BLOCK_PASS) - 1) * BLOCK_PASS, 4))


def workspace_bytes(B, M, N, h, w):
    return cdiv(B * (M + N) * chunk_plan(h * w).chunks * 3 * 4, 256) * 256


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------
def finalize_tail(fn, B, M, N, hw, tot_a, tot_p, la, ca, lp, cp, le, weights):
    """The thread-0 tail of k_loss_finalize in Python floats (IEEE double, the kernel's order of operations): the 8 outputs in double.
    tot_g = (sum0, sum1, count) of one heatmap group as k_loss_hm_partial defines them."""
    hm_w, off_w, emb_w = (f32(v) for v in weights)
    hm = 0.0
    for (t0, t1, t2), Cg in ((tot_a, M), (tot_p, N)):
        n_el = float(B) * Cg * hw
        if fn == "mse":
            hm += t0 / n_el
        else:
            hm += -t0 if t2 == 0.0 else -(t1 + t0) / t2
    hm *= hm_w
    off = off_w * ((la / ca if ca > 0 else 0.0) + (lp / cp if cp > 0 else 0.0))
    emb = emb_w * (le / cp if cp > 0 else 0.0)
    return np.array([hm + off + emb, hm, off, emb, tot_a[2], tot_p[2], ca, cp], np.float64)


def _l1(feat, tgt, inds, mask, hw):
    """feat (B, 2, hw) double; the ABI clamps indices to [0, hw - 1].  -> (sum, count, clamped ids, sign of pred - target, masked)."""
    ids = inds.long().clamp(0, hw - 1)
    g = feat.gather(2, ids[:, None, :].expand(-1, 2, -1)).permute(0, 2, 1)
    diff = g - tgt.double()
    m = mask.bool()
    return float((diff.abs() * m[..., None]).sum()), float(m.sum()), ids, torch.sign(diff) * m[..., None]


def loss_reference(head, targets, M, N, fn="mse", weights=DEFAULT_WEIGHTS, grad_out=1.0):
    """Loss.forward of the reference and its gradient in float64 on the float32 inputs: head (B, M + N + 4, h, w), the Encode targets.
    Returns out8 (double: total, hm, offset, embedding, num_pos_a, num_pos_p, n_valid_a, n_valid_p; the num_pos are 0 under mse, which
    does not count them), dhead = grad_out * d total / d head, and `sat`, the heatmap cells whose sigmoid the clamp cuts off."""
    x = head.double()
    B, C4, h, w = x.shape
    hw, C = h * w, M + N
    hm_w, off_w, emb_w = (f32(v) for v in weights)
    go = f32(grad_out)
    sr = 1.0 / (1.0 + torch.exp(-x[:, :C]))
    passed = (sr >= CLAMP_LO) & (sr <= CLAMP_HI)                     # clamp backward: inclusive bounds
    s = sr.clamp(CLAMP_LO, CLAMP_HI)
    t = torch.cat([targets["anchor_hm"], targets["part_hm"]], 1).double()
    tots, d = [], torch.zeros_like(s)
    for sl, Cg in ((slice(0, M), M), (slice(M, C), N)):
        sg, tg = s[:, sl], t[:, sl]
        if fn == "mse":
            tots.append((float(((sg - tg) ** 2).sum()), 0.0, 0.0))
            d[:, sl] = (go * hm_w) * 2.0 / (float(B) * Cg * hw) * (sg - tg)
        else:
            pos, neg = tg == 1, tg < 1
            w4 = (1.0 - tg) ** 4
            neg_sum = float((torch.log(1.0 - sg) * sg * sg * w4 * neg).sum())
            pos_sum = float((torch.log(sg) * (1.0 - sg) ** 2 * pos).sum())
            npos = float(pos.sum())
            tots.append((neg_sum, pos_sum, npos))
            dls = (2.0 * sg * torch.log(1.0 - sg) - sg * sg / (1.0 - sg)) * w4 * neg
            if npos:
                dls = dls + ((1.0 - sg) ** 2 / sg - 2.0 * (1.0 - sg) * torch.log(sg)) * pos
            d[:, sl] = -(go * hm_w) / (npos if npos else 1.0) * dls
    d = d * passed * sr * (1.0 - sr)
    reg = x[:, C:].reshape(B, 4, hw)
    la, ca, ia, sa = _l1(reg[:, 0:2], targets["anchor_offsets"], targets["anchor_inds"], targets["anchor_mask"], hw)
    lp, cp, ip, sp = _l1(reg[:, 0:2], targets["part_offsets"], targets["part_inds"], targets["part_mask"], hw)
    le, _, _, se = _l1(reg[:, 2:4], targets["embeddings"], targets["part_inds"], targets["part_mask"], hw)
    dreg = torch.zeros(B, 4, hw, dtype=torch.float64)
    for ch0, ids, sign, wgt, cnt in ((0, ia, sa, off_w, ca), (0, ip, sp, off_w, cp), (2, ip, se, emb_w, cp)):
        if cnt > 0:
            for j in (0, 1):
                dreg[:, ch0 + j].scatter_add_(1, ids, sign[..., j] * (go * wgt / cnt))
    out8 = finalize_tail(fn, B, M, N, hw, tots[0], tots[1], la, ca, lp, cp, le, weights)
    return SimpleNamespace(out8=out8, dhead=torch.cat([d, dreg.view(B, 4, h, w)], 1), sat=~passed)


def deviations(ref, got4, got_grad, targets, M, N):
    """The error classes of the module docstring of one result (fp32 oracle or kernel) against `ref`; inf where a reference of exactly 0
    (an all-masked L1 term, an empty gradient group) is not met exactly."""
    C = M + N
    out = {"value": 0.0}
    for i in range(4):
        r, g = float(ref.out8[i]), float(got4[i])
        e = abs(g - r) / abs(r) if r != 0 else (0.0 if g == 0 else float("inf"))
        out["value"] = max(out["value"], e) if np.isfinite(g) else float("inf")
    err = (got_grad.double() - ref.dhead).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    err[:, :C] = err[:, :C].masked_fill(ref.sat, 0.0)
    mag = ref.dhead.abs()
    mag[:, :C] = mag[:, :C].masked_fill(ref.sat, 0.0)

    def ratio(e, m):
        if e.numel() == 0:
            return 0.0
        e, m = float(e.max()), float(m.max())
        return e / m if m > 0 else (0.0 if e == 0 else float("inf"))

    for name, sl in zip(GROUPS, (slice(0, M), slice(M, C), slice(C, C + 2), slice(C + 2, C + 4))):
        out[name] = ratio(err[:, sl], mag[:, sl])
    pos = (torch.cat([targets["anchor_hm"], targets["part_hm"]], 1) == 1) & ~ref.sat
    out["positives"] = ratio(err[:, :C][pos], mag[:, :C][pos])
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _targets(a_hm, p_hm, a_inds, p_inds, a_off, p_off, emb, a_mask, p_mask):
    return {"anchor_hm": a_hm, "part_hm": p_hm, "anchor_inds": a_inds, "part_inds": p_inds, "anchor_offsets": a_off, "part_offsets": p_off,
            "embeddings": emb, "anchor_mask": a_mask, "part_mask": p_mask}


def random_case(B, M, N, h, w, K=5, P=7, seed=0, peaks="both", all_masked=False):
    """The random regime (module docstring).  Peaks sit at even positions with a nextafter(1, 0) neighbour to their right; every plane
    of hw >= 100 carries min(6, hw // 100) saturated logits, cycled through SATURATED so that every value occurs."""
    g = _gen(seed)
    hw, C = h * w, M + N
    head = torch.empty(B, C + 4, hw)
    head[:, :C] = torch.rand(B, C, hw, generator=g) * 8 - 4
    head[:, C:] = torch.randn(B, 4, hw, generator=g)
    t = torch.rand(B, C, hw, generator=g)
    assert float(t.max()) < 1.0
    n_sat = min(len(SATURATED), hw // 100)
    assert n_sat <= SAT_SHARE_CAP * hw
    planted = torch.zeros(B, C, hw, dtype=torch.bool)
    for b in range(B):
        for c in range(C):
            if peaks == "both" or peaks == ("anchor" if c < M else "part"):
                at = torch.randperm(hw // 2, generator=g)[:1 + hw // 1000] * 2
                t[b, c, at] = 1.0
                t[b, c, at + 1] = BELOW_ONE
            at = torch.randperm(hw, generator=g)[:n_sat]
            head[b, c, at] = torch.tensor([SATURATED[(b * C + c + j) % len(SATURATED)] for j in range(n_sat)])
            planted[b, c, at] = True
    a_mask = torch.rand(B, K, generator=g) < 0.7
    p_mask = torch.rand(B, P, generator=g) < 0.7
    a_mask[0, 0] = p_mask[0, 0] = True
    if all_masked:
        a_mask[:], p_mask[:] = False, False
    tg = _targets(t[:, :M].reshape(B, M, h, w).clone(), t[:, M:].reshape(B, N, h, w).clone(),
                  torch.randint(0, hw, (B, K), generator=g), torch.randint(0, hw, (B, P), generator=g),
                  torch.rand(B, K, 2, generator=g), torch.rand(B, P, 2, generator=g), torch.randn(B, P, 2, generator=g) * 3, a_mask, p_mask)
    return SimpleNamespace(head=head.view(B, C + 4, h, w), targets=tg, B=B, M=M, N=N, h=h, w=w, K=K, P=P, planted=planted.view(B, C, h, w),
                           weights=DEFAULT_WEIGHTS)


@functools.lru_cache(maxsize=None)
def case_table():
    """SHAPES x B in {1, 3} x (M, N) in {(1,1), (2,1), (3,5)}, the peak configurations and an all-masked list cycled through them, and
    one case whose B * (M + N) * chunks = 320 partials need the finalize's second stride."""
    cases, i = {}, 0
    for name, (h, w) in SHAPES.items():
        for B in (1, 3):
            for M, N in ((1, 1), (2, 1), (3, 5)):
                cases[f"{name}-b{B}-m{M}n{N}"] = dict(B=B, M=M, N=N, h=h, w=w, seed=100 + i, peaks=PEAKS[(i + i // 4) % 4], all_masked=i % 7 == 5)
                i += 1
    cases["finalize_stride_320_partials-b20-m3n5"] = dict(B=20, M=3, N=5, h=89, w=92, seed=99, peaks="both", all_masked=False)
    return cases


@functools.lru_cache(maxsize=None)
def table_case(name):
    return random_case(**case_table()[name])


@functools.lru_cache(maxsize=None)
def table_reference(name, fn):
    """The fp64 reference of a table case at grad_out = 1: computed once, shared, never modified."""
    c = table_case(name)
    return loss_reference(c.head, c.targets, c.M, c.N, fn, c.weights, 1.0)


def _dyadic(g, shape, span=32, step=8):
    return torch.randint(-span, span + 1, tuple(shape), generator=g).float() / step


def exact_case(B, M, N, h, w, K=6, P=9, seed=0):
    """The exact regime: logits 0, targets from {0, 1/4, 1/2, 3/4, 1}, regression values and their targets multiples of 1/8 in [-4, 4],
    duplicates within and across the lists, one entry per list whose prediction equals its target (dx == 0)."""
    g = _gen(seed)
    hw, C = h * w, M + N
    head = torch.zeros(B, C + 4, hw)
    head[:, C:] = _dyadic(g, (B, 4, hw))
    t = torch.randint(0, 5, (B, C, h, w), generator=g).float() / 4
    a_inds, p_inds = torch.randint(0, hw, (B, K), generator=g), torch.randint(0, hw, (B, P), generator=g)
    a_inds[:, 1] = a_inds[:, 0]
    p_inds[:, 0] = a_inds[:, 0]
    a_off, p_off, emb = _dyadic(g, (B, K, 2)), _dyadic(g, (B, P, 2)), _dyadic(g, (B, P, 2))
    bi = torch.arange(B)
    a_off[:, 2] = head[bi, C:C + 2, a_inds[:, 2]]
    p_off[:, 2] = head[bi, C:C + 2, p_inds[:, 2]]
    emb[:, 3] = head[bi, C + 2:C + 4, p_inds[:, 3]]
    a_mask, p_mask = torch.rand(B, K, generator=g) < 0.7, torch.rand(B, P, generator=g) < 0.7
    a_mask[:, :3] = True
    p_mask[:, :4] = True
    tg = _targets(t[:, :M].clone(), t[:, M:].clone(), a_inds, p_inds, a_off, p_off, emb, a_mask, p_mask)
    return SimpleNamespace(head=head.view(B, C + 4, h, w), targets=tg, B=B, M=M, N=N, h=h, w=w, K=K, P=P, weights=EXACT_WEIGHTS)


def exact_sums(case):
    """(tot_a, tot_p, la, ca, lp, cp, le) of an exact-regime case under mse, from integer arithmetic: every term is a multiple of 1/16
    (heatmaps) or 1/8 (L1), so the int64 sums are the true sums."""
    M, C, hw = case.M, case.M + case.N, case.h * case.w
    t = torch.cat([case.targets["anchor_hm"], case.targets["part_hm"]], 1).double()
    q = ((0.5 - t) ** 2 * 16).round().long()
    tots = [(float(q[:, sl].sum()) / 16, 0.0, 0.0) for sl in (slice(0, M), slice(M, C))]
    reg = case.head[:, C:].reshape(case.B, 4, hw).double()
    tg = case.targets
    out = []
    for ch0, key, who in ((0, "anchor_offsets", "anchor"), (0, "part_offsets", "part"), (2, "embeddings", "part")):
        s, c, _, _ = _l1(reg[:, ch0:ch0 + 2], tg[key], tg[f"{who}_inds"], tg[f"{who}_mask"], hw)
        assert s * 8 == round(s * 8)
        out += [s, c]
    la, ca, lp, cp, le, _ = out
    return tots[0], tots[1], la, ca, lp, cp, le


def exact_out8(case, B=None):
    """What sd_loss_fwd must return for an exact-regime case under mse, bit for bit."""
    return finalize_tail("mse", case.B if B is None else B, case.M, case.N, case.h * case.w, *exact_sums(case), case.weights).astype(np.float32)


def mse_scale_f32(go, hm_w, B, Cg, hw):
    """`scale` of k_loss_bwd_dense under mse in numpy float32, the kernel's order: (go * hm_w) * 2 / ((B * Cg) * hw)."""
    f = np.float32
    return (f(go) * f(hm_w)) * f(2.0) / ((f(B) * f(Cg)) * f(hw))


def scatter_weights_f32(go, off_w, emb_w, ca, cp):
    """wa, wp, we of k_loss_bwd_scatter in numpy float32: go * w / count, 0 for an empty list; the embedding count is the part count."""
    f = np.float32
    return (f(go) * f(off_w) / f(ca) if ca > 0 else f(0), f(go) * f(off_w) / f(cp) if cp > 0 else f(0), f(go) * f(emb_w) / f(cp) if cp > 0 else f(0))


def scatter_expected(case, go, reverse=False):
    """The four regression channels of dhead, (B, 4, hw) float32: per cell the float32 sum, in list order (anchors, then parts), of
    sign(pred - target) * w over the masked entries whose clamped index is that cell; 0 everywhere else.  reverse = the other order."""
    f = np.float32
    B, C, hw = case.B, case.M + case.N, case.h * case.w
    tg = {k: v.numpy() for k, v in case.targets.items()}
    ca, cp = int(tg["anchor_mask"].sum()), int(tg["part_mask"].sum())
    wa, wp, we = scatter_weights_f32(go, case.weights[1], case.weights[2], ca, cp)
    reg = case.head.numpy().reshape(B, C + 4, hw)[:, C:]
    out = np.zeros((B, 4, hw), np.float32)
    for b in range(B):
        for ch0, lists in ((0, (("anchor", "anchor_offsets", wa), ("part", "part_offsets", wp))), (2, (("part", "embeddings", we),))):
            entries = [(min(max(int(tg[f"{who}_inds"][b, e]), 0), hw - 1), tg[key][b, e], wgt)
                       for who, key, wgt in lists for e in range(tg[f"{who}_inds"].shape[1]) if tg[f"{who}_mask"][b, e]]
            cells = {}
            for idx, target, wgt in (reversed(entries) if reverse else entries):
                for j in (0, 1):
                    dlt = f(reg[b, ch0 + j, idx]) - f(target[j])
                    v = wgt if dlt > 0 else (-wgt if dlt < 0 else f(0))
                    cells[(idx, j)] = f(cells[(idx, j)] + v) if (idx, j) in cells else v
            for (idx, j), v in cells.items():
                out[b, ch0 + j, idx] = v
    return out


def exact_dhead(case, go):
    """What sd_loss_bwd must write for an exact-regime case under mse, bit for bit: scale * (0.5 - t) * 0.25 on the heatmap channels
    (dls and sr (1 - sr) are powers of two or their small multiples: both products are exact), scatter_expected on the other four."""
    f = np.float32
    B, M, N, h, w = case.B, case.M, case.N, case.h, case.w
    t = torch.cat([case.targets["anchor_hm"], case.targets["part_hm"]], 1).numpy()
    d = np.empty((B, M + N + 4, h, w), np.float32)
    for sl, Cg in ((slice(0, M), M), (slice(M, M + N), N)):
        d[:, sl] = mse_scale_f32(go, case.weights[0], B, Cg, h * w) * (f(0.5) - t[:, sl]) * f(0.25)
    d[:, M + N:] = scatter_expected(case, go).reshape(B, 4, h, w)
    return d


def sweep_positions(hw):
    return sorted({0, 3, 4, 1020, 1023, 1024, 4092, 4095, 4096, hw - 4, hw - 1})


def onehot_sweep(M, N, h, w):
    """One image per (channel, position): t = 0.5 everywhere (term 0) except t = 1 at that one element (term 1/4); first and last channel
    of each group.  Row b of sd_loss_fwd_per_image must be fp32(0.25 / (Cg * hw)) in [total, hm] and 0 elsewhere."""
    hw, C = h * w, M + N
    where = [(c, p) for c in sorted({0, M - 1, M, C - 1}) for p in sweep_positions(hw)]
    B = len(where)
    t = torch.full((B, C, hw), 0.5)
    for b, (c, p) in enumerate(where):
        t[b, c, p] = 1.0
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    tg = _targets(t[:, :M].reshape(B, M, h, w).clone(), t[:, M:].reshape(B, N, h, w).clone(), z(B, 1, dt=torch.int64), z(B, 1, dt=torch.int64),
                  z(B, 1, 2), z(B, 1, 2), z(B, 1, 2), z(B, 1, dt=torch.bool), z(B, 1, dt=torch.bool))
    rows = np.zeros((B, 8), np.float32)
    for b, (c, p) in enumerate(where):
        one = ((0.25, 0.0, 0.0), (0.0, 0.0, 0.0)) if c < M else ((0.0, 0.0, 0.0), (0.25, 0.0, 0.0))
        rows[b] = finalize_tail("mse", 1, M, N, hw, one[0], one[1], 0.0, 0.0, 0.0, 0.0, 0.0, EXACT_WEIGHTS).astype(np.float32)
    case = SimpleNamespace(head=torch.zeros(B, C + 4, h, w), targets=tg, B=B, M=M, N=N, h=h, w=w, K=1, P=1, weights=EXACT_WEIGHTS)
    return case, where, rows


# ---- hand-made scatter cases ------------------------------------------------------------------------------------------------------
def blank_case(B, M, N, h, w, K, P, seed=0):
    """Logits 0, targets 0.5, dyadic regression predictions, every list entry masked off at index 0 with the prediction as its target."""
    g = _gen(seed)
    hw, C = h * w, M + N
    head = torch.zeros(B, C + 4, hw)
    head[:, C:] = _dyadic(g, (B, 4, hw))
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    tg = _targets(torch.full((B, M, h, w), 0.5), torch.full((B, N, h, w), 0.5), z(B, K, dt=torch.int64), z(B, P, dt=torch.int64),
                  z(B, K, 2), z(B, P, 2), z(B, P, 2), z(B, K, dt=torch.bool), z(B, P, dt=torch.bool))
    return SimpleNamespace(head=head.view(B, C + 4, h, w), targets=tg, B=B, M=M, N=N, h=h, w=w, K=K, P=P, weights=EXACT_WEIGHTS)


def put(case, who, e, idx, sign=(1, 1), esign=None, mask=True, b=0):
    """List entry e of `who` (anchor / part) at cell idx with sign(pred - target) = sign (embedding: esign, default sign); the target is
    the prediction at the clamped cell minus the sign, so the difference is exactly +-1 or 0."""
    hw, C = case.h * case.w, case.M + case.N
    cell = min(max(idx, 0), hw - 1)
    reg = case.head.view(case.B, C + 4, hw)[b, C:, cell]
    tg = case.targets
    tg[f"{who}_inds"][b, e] = idx
    tg[f"{who}_mask"][b, e] = mask
    tg[f"{who}_offsets"][b, e] = reg[0:2] - torch.tensor(sign, dtype=torch.float32)
    if who == "part":
        tg["embeddings"][b, e] = reg[2:4] - torch.tensor(sign if esign is None else esign, dtype=torch.float32)


def _single_signs():
    c = blank_case(1, 2, 1, 16, 24, 4, 4, 1)
    put(c, "anchor", 0, 5, (1, -1)); put(c, "anchor", 1, 9, (0, 0)); put(c, "anchor", 2, 13, (-1, 0))
    put(c, "part", 0, 20, (-1, 1), (0, -1)); put(c, "part", 1, 21, (0, 1), (1, 0))
    return c


def _two_anchors_one_cell():
    c = blank_case(1, 2, 1, 16, 24, 4, 4, 2)
    put(c, "anchor", 0, 7, (1, 1)); put(c, "anchor", 1, 7, (1, -1)); put(c, "anchor", 3, 8, (-1, -1))
    put(c, "part", 2, 30, (1, 1))
    return c


def _anchor_part_cancel():
    c = blank_case(1, 2, 1, 16, 24, 4, 4, 3)
    put(c, "anchor", 0, 11, (1, -1)); put(c, "anchor", 1, 50, (1, 1))
    put(c, "part", 0, 11, (-1, 1)); put(c, "part", 1, 60, (-1, -1))
    return c


def _anchor_part_differ():
    c = blank_case(1, 2, 1, 16, 24, 4, 4, 4)
    put(c, "anchor", 0, 11, (1, -1)); put(c, "anchor", 1, 50, (1, 1)); put(c, "anchor", 2, 51, (1, 1))
    put(c, "part", 0, 11, (1, 1)); put(c, "part", 1, 60, (-1, -1))
    return c


def _three_duplicates_list_order():
    """ca = 3, cp = 7: wa = fp32(1/6), wp = fp32(1/14), we = fp32(1/28).  Cells with one anchor and two to four parts, same and mixed
    signs: the float32 sum depends on the order (tests/test_loss_ref_cpu.py asserts that it does in at least one cell)."""
    c = blank_case(1, 2, 1, 16, 24, 3, 7, 5)
    put(c, "anchor", 0, 40, (1, 1)); put(c, "anchor", 1, 90, (1, -1)); put(c, "anchor", 2, 91, (-1, -1))
    put(c, "part", 0, 40, (1, 1)); put(c, "part", 1, 40, (1, -1), (1, 1))
    put(c, "part", 2, 90, (1, 1)); put(c, "part", 3, 90, (1, 1)); put(c, "part", 4, 90, (1, 1), (-1, 1)); put(c, "part", 5, 90, (1, -1))
    put(c, "part", 6, 91, (-1, 1))
    return c


def _masked_off_duplicate():
    c = blank_case(1, 2, 1, 16, 24, 4, 4, 6)
    put(c, "anchor", 0, 70, (1, 1)); put(c, "anchor", 1, 70, (1, 1), mask=False); put(c, "anchor", 2, 71, (-1, 1))
    put(c, "part", 0, 70, (1, 1), mask=False); put(c, "part", 1, 72, (1, 1)); put(c, "part", 2, 72, (-1, -1), mask=False)
    return c


def _index_clamp():
    c = blank_case(1, 2, 1, 16, 24, 4, 4, 7)
    hw = 384
    put(c, "anchor", 0, -5, (1, 1)); put(c, "anchor", 1, hw + 7, (-1, 1)); put(c, "anchor", 2, 100, (1, 1))
    put(c, "part", 0, -1, (1, -1)); put(c, "part", 1, hw + 100, (-1, -1))
    return c


def _all_masks_off():
    c = blank_case(2, 2, 1, 16, 24, 4, 4, 8)
    for b in (0, 1):
        put(c, "anchor", 0, 5, (1, 1), mask=False, b=b); put(c, "part", 1, 9, (-1, 1), mask=False, b=b)
    return c


def _structured(B, K, P, seed, a_cell, p_cell):
    c = blank_case(B, 2, 1, 16, 24, K, P, seed)
    for b in range(B):
        for e in range(K):
            put(c, "anchor", e, a_cell(b, e), ((e + b) % 3 - 1, (e // 3) % 3 - 1), b=b)
        for e in range(P):
            put(c, "part", e, p_cell(b, e), ((e // 2) % 3 - 1, (e + 1 + b) % 3 - 1), ((e + 2) % 3 - 1, e % 3 - 1), b=b)
    return c


def _k200_p120_across_256():
    """Offsets list entries 0..319: duplicates (anchor 10, part 100 = entry 300), (parts 50 and 70 = entries 250 and 270) and (anchor 5,
    part 119 = entry 319) have one member on each side of the scatter loop's stride of 256."""
    dup = {100: 10, 70: 250, 119: 5}
    return _structured(1, 200, 120, 9, lambda b, e: e, lambda b, e: dup.get(e, 200 + e))


def _p300_embedding_stride():
    dup = {299: 3 + 4, 280: 260 + 4}
    return _structured(1, 4, 300, 10, lambda b, e: e, lambda b, e: dup.get(e, 4 + e))


def _l1_term_b3_k100():
    return _structured(3, 100, 7, 11, lambda b, e: (e * 3 + b) % 384, lambda b, e: (e * 5 + 2 * b) % 384)


SCATTER_CASES = {
    "single_entry_signs": _single_signs, "two_anchors_one_cell": _two_anchors_one_cell, "anchor_part_cancel_to_zero": _anchor_part_cancel,
    "anchor_part_different_weights": _anchor_part_differ, "three_duplicates_list_order": _three_duplicates_list_order,
    "masked_off_duplicate_ignored": _masked_off_duplicate, "index_clamp_minus5_hw_plus7": _index_clamp, "all_masks_off": _all_masks_off,
    "k200_p120_duplicates_across_256": _k200_p120_across_256, "p300_embedding_stride": _p300_embedding_stride,
    "l1_term_b3_k100_stride": _l1_term_b3_k100,
}


# ---- target rendering --------------------------------------------------------------------------------------------------------------
def min_d2(cx, cy, h, w):
    """(h, w) int64 min over the keypoints of (x - cx)^2 + (y - cy)^2; None for an empty channel."""
    if len(cx) == 0:
        return None
    Y, X = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    best = None
    for i in range(0, len(cx), 16):      # blocks of keypoints: (16, h, w) int64 at the most
        d = (X[None] - np.asarray(cx[i:i + 16], np.int64)[:, None, None]) ** 2 + (Y[None] - np.asarray(cy[i:i + 16], np.int64)[:, None, None]) ** 2
        d = d.min(0)
        best = d if best is None else np.minimum(best, d)
    return best


def render_reference(d2, two_sigma2):
    """exp in float64 of the float32 quotient fp32(-d^2) / fp32(2 sigma^2); an empty channel is 0."""
    q = (-d2).astype(np.float32) / np.float32(two_sigma2)
    return np.exp(q.astype(np.float64))
