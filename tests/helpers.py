"""Shared helpers for the parity tests (data plumbing only)."""
import numpy as np


def scene_from_flat(objs, parts):
    """Inverse of gen_goldens.flat_scene: -> [(label, x, y, [(kind, x, y), ...]), ...]."""
    out, j = [], 0
    for (l, x, y, n) in objs:
        ps = [(int(parts[j + i][0]), float(parts[j + i][1]), float(parts[j + i][2])) for i in range(int(n))]
        j += int(n)
        out.append((int(l), float(x), float(y), ps))
    return out


def objects_to_arrays(objs):
    """oracle.assemble_objects output -> (n,4) [label,x,y,score], (m,5) [obj,kind,x,y,score]."""
    o = np.array([[l, a[0], a[1], a[2]] for (l, a, _) in objs], np.float64).reshape(-1, 4)
    p = np.array([[i, k, x, y, s] for i, (_, _, ps) in enumerate(objs) for (k, x, y, s) in ps], np.float64).reshape(-1, 5)
    return o, p


ENC_KEYS = ["anchor_hm", "part_hm", "anchor_inds", "part_inds", "anchor_offsets", "part_offsets",
            "embeddings", "anchor_mask", "part_mask"]


# ---------------------------------------------------------------------------------------------
# BASELINE configs[0]: 16 synthetic samples on disk (PNG + JSON, README.md:40-71 schema with "box": null)
# ---------------------------------------------------------------------------------------------
EVAL16_LABELS = {"bean": 0, "maize": 1}
EVAL16_PARTS = {"leaf": 0}


def write_evaluate16_dir(g, directory):
    """Materialise the scenes of tests/golden/evaluate16.npz as img_NN.png + img_NN.json under `directory`
    (image sizes as recorded; blocky seeded-noise content) and return the 16 planted head tensors (7, 128, 128),
    carried by the golden in quantised form."""
    import json
    from pathlib import Path

    from PIL import Image

    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    W, H, M, N, K, P = (int(v) for v in g["cfg"])
    rl = {v: k for k, v in EVAL16_LABELS.items()}
    rp = {v: k for k, v in EVAL16_PARTS.items()}
    heads = []
    for n in range(16):
        iw, ih = (int(v) for v in g[f"size{n}"])
        objs = scene_from_flat(g[f"scene{n}_objs"], g[f"scene{n}_parts"])
        rng = np.random.default_rng(100 + n)
        small = rng.integers(0, 256, (ih // 16, iw // 16, 3), dtype=np.uint8)
        Image.fromarray(np.repeat(np.repeat(small, 16, 0), 16, 1)).save(directory / f"img_{n:02d}.png")
        js = {"image_path": str(directory / f"img_{n:02d}.png"), "img_size": [iw, ih],
              "objects": [{"label": rl[l], "box": None,
                           "parts": [{"kind": "stem", "location": {"x": x, "y": y}}]
                           + [{"kind": rp[k], "location": {"x": px, "y": py}} for (k, px, py) in ps]}
                          for (l, x, y, ps) in objs]}
        (directory / f"img_{n:02d}.json").write_text(json.dumps(js))
        # the planted head tensors travel in the fixture (exp / log differ by an ulp between host CPUs): int16 logits on a
        # 1/1024 grid, int8 regression channels on a 1/16 grid, the planted offset / embedding cells in full fp32
        reg = (g[f"head{n}_reg_q16"].astype(np.float32) / np.float32(16)).reshape(4, -1)
        reg[:, g[f"head{n}_cells"]] = g[f"head{n}_cell_vals"].T
        head = np.concatenate([g[f"head{n}_hm_q1024"].astype(np.float32) / np.float32(1024), reg.reshape(4, H // 4, W // 4)], 0)
        heads.append(head)
    return heads


def assert_evaluator_equals_golden(ev, g):
    for sec, evals in (("anchor", ev.anchor_eval), ("part", ev.part_eval), ("csi", ev.csi_eval), ("classif", ev.classification_eval)):
        assert list(evals.labels) == list(g[f"{sec}_labels"])
        counts = np.array([[e.tp, e.npos, e.ndet] for _, e in evals.items()], np.int64)
        np.testing.assert_array_equal(counts, g[f"{sec}_counts"], err_msg=sec)
        for label, e in evals.items():
            np.testing.assert_array_equal(np.array(e.acc, np.float64), g[f"{sec}_acc_{label}"], err_msg=f"{sec} {label}")
    assert ev._csv_kps_str() == str(g["csv"])


# ---------------------------------------------------------------------------------------------
# decoder parity: HIP packed result vs oracle.decode_tensors
# ---------------------------------------------------------------------------------------------
def safe_ranks(es, rel=2e-6):
    """Ranks whose score is separated from both neighbours by more than `rel` (relative): GPU and CPU sigmoids differ by a
    few ulp, so only there is the rank -> peak mapping defined identically on both sides."""
    es = np.asarray(es)
    gap = np.abs(np.diff(es.astype(np.float64), axis=1)) / np.maximum(es[:, 1:], 1e-30)
    safe = np.ones_like(es, bool)
    safe[:, 1:] &= gap > rel
    safe[:, :-1] &= gap > rel
    return safe


def assert_decode_matches_oracle(got, t, conf, sig_tol):
    """got = Decoder.split_packed(...) (numpy), t = oracle.decode_tensors(...).  Bit-exact where the ranking is defined:
      * per safe rank: flat index, class, refined x / y (same fp32 adds), gathered embedding; scores to `sig_tol`;
      * grouping, UNCONDITIONALLY for every safe part rank: the part is attached to the same anchor PEAK (class, flat index)
        or to none on both sides -- comparing the anchor's identity instead of its rank keeps the assertion meaningful when
        two near-tied anchors swap ranks;
      * in images whose above-threshold anchors are all safe, additionally the raw `assign` rank array.
    Returns (parts checked, parts total, images with the strict rank check)."""
    conf32 = np.float32(conf)
    safe = {}
    for grp in ("anchor", "part"):
        es = t[f"{grp}_out"][..., 2]
        s = safe[grp] = safe_ranks(es)
        np.testing.assert_array_equal(got[f"{grp}_ind"][s], t[f"{grp}_inds"][s])
        for ch in (3, 0, 1):
            np.testing.assert_array_equal(got[f"{grp}_out"][..., ch][s], t[f"{grp}_out"][..., ch][s])
        np.testing.assert_allclose(got[f"{grp}_out"][..., 2], es, **sig_tol)
    ps = safe["part"]
    np.testing.assert_array_equal(got["part_emb"][ps], t["part_embeddings"][ps])
    np.testing.assert_array_equal(got["part_out"][..., 4:6][ps], t["part_out"][..., 4:6][ps])
    B, P = ps.shape
    want_assign = np.where(t["valid"], t["min_inds"], -1)
    bi = np.arange(B)[:, None]

    def identity(assign, a_ind, a_cls):
        a = np.maximum(assign, 0)
        ident = a_cls[bi, a].astype(np.int64) * (1 << 32) + a_ind[bi, a].astype(np.int64)
        return np.where(assign >= 0, ident, -1)

    id_got = identity(got["assign"], got["anchor_ind"], got["anchor_out"][..., 3])
    id_want = identity(want_assign, t["anchor_inds"], t["anchor_out"][..., 3])
    np.testing.assert_array_equal(id_got[ps], id_want[ps])
    strict = 0
    for b in range(B):
        live = t["anchor_out"][b, :, 2] > conf32
        if safe["anchor"][b][live].all():
            np.testing.assert_array_equal(got["assign"][b][ps[b]], want_assign[b][ps[b]])
            strict += 1
    return int(ps.sum()), int(ps.size), strict


# ---------------------------------------------------------------------------------------------
# per-layer operands of an oracle run (tests/test_gpu_production_parity.py)
# ---------------------------------------------------------------------------------------------
def oracle_conv_trace(ref, x, dhead_of, device, skip=()):
    """Run `ref(x)` (torch-CPU oracle network, training mode) and its backward from `dhead_of(head)`, capturing for every
    Conv2d the tensors that layer saw: input x, output y, output gradient dy and input gradient dx (None where the input needs
    no gradient), each moved to `device` as a contiguous NHWC tensor.  Returns (head.detach(), {module name: dict})."""
    import torch
    trace, handles = {}, []

    def nhwc(t):
        return t.detach().permute(0, 2, 3, 1).contiguous().to(device)

    for name, m in ref.named_modules():
        if not isinstance(m, torch.nn.Conv2d) or name in skip:
            continue
        rec = trace[name] = {"module": m}

        def fwd_hook(mod, inp, out, rec=rec):
            rec["x"], rec["y"] = nhwc(inp[0]), nhwc(out)

        def bwd_hook(mod, gin, gout, rec=rec):
            rec["dy"] = nhwc(gout[0])
            rec["dx"] = nhwc(gin[0]) if gin[0] is not None else None

        handles.append(m.register_forward_hook(fwd_hook))
        handles.append(m.register_full_backward_hook(bwd_hook))
    try:
        head = ref(x)
        head.backward(dhead_of(head))
    finally:
        for h in handles:
            h.remove()
    return head.detach(), trace


# ---------------------------------------------------------------------------------------------
# bit-exact conv / head tests (tests/test_exact_cases_cpu.py, tests/test_gpu_exact.py)
#
# Integer operands make every product and every partial sum of a conv an integer.  While the sum of the ABSOLUTE products stays below
# 2^24, every partial sum -- in any order, with or without FMA, for any tile, split, ring or reduce pass -- is an integer below 2^24 and
# therefore exact in fp32: an fp32 kernel must reproduce the fp64 reference bit for bit, a bf16 kernel its nearest-even rounding.
# Epilogues add half-integer shifts and scales of 0.5 / 1 / 2: multiples of 0.5 are exact in fp32 below 2^23, the limit used there.
# ---------------------------------------------------------------------------------------------
EXACT_LIMIT = float(2 ** 24)
EXACT_LIMIT_HALVES = float(2 ** 23)
MAX_REFERENCE_MACS = 2 ** 31

# library defaults of the thread-local dispatch options the cases change (include/sdnet_hip.h, sd_set_option)
OPTION_DEFAULTS = {"conv_patch_min_tiles": 512, "conv_pp_min_tiles": 200, "conv_rows64_min_units": 192, "conv_rows_f32_min_units": 192,
                   "conv_fwd_split_k": 1, "conv_patch_narrow": 2, "conv_pp_strips": 1, "conv_rows16": 1, "igemm_big_bf16": 0,
                   "conv1x1_stream_min_pixels": 32 * 2048, "conv_patch_bn64": 0, "wgrad_f32_ring": 2, "wgrad_bf16_ring": 5}


class dispatch_options:
    """with dispatch_options(lib, {...}): sets the thread-local options and restores the defaults on the way out."""

    def __init__(self, lib, opts):
        self.lib, self.opts = lib, dict(opts)

    def __enter__(self):
        for k, v in self.opts.items():
            assert self.lib.sd_set_option(k.encode(), int(v)) == 0, k
        return self

    def __exit__(self, *exc):
        for k in self.opts:
            assert self.lib.sd_set_option(k.encode(), OPTION_DEFAULTS[k]) == 0, k
        return False


def conv_desc(L, geom):
    B, H, W, cin, cout, k, stride, pad = geom
    d = L.ConvDesc()
    d.B, d.Hi, d.Wi, d.Cin, d.Cout, d.R, d.S, d.stride, d.pad = B, H, W, cin, cout, k, k, stride, pad
    d.Ho, d.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return d


def conv_macs(geom):
    B, H, W, cin, cout, k, stride, pad = geom
    return B * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1) * cin * cout * k * k


# (geometry (B, H, W, Cin, Cout, k, stride, pad), options, {sd_conv2d_kernel_name pass: kernel the case must reach}).  Passes 0 / 1 / 2 =
# fp32 forward / data-gradient / weight gradient, 16 / 17 = bf16 forward / data-gradient.  The geometries are those of the tolerance tests
# (CONV_CASES, PATCH_CASES, the row-stream, two-group and 1x1-stream cases of tests/test_gpu_network.py and tests/test_gpu_amp.py) without
# the ones whose reference costs more than 2^31 multiply-adds, kernels behind size thresholds reached through the options.
# k_conv_igemm_big has no threshold option: its plan needs 512 tiles of 256 x 128 outputs and a reduction of at least 512, i.e. 2^33
# multiply-adds for the unit-stride form -- the one 1x1 case (a plain GEMM for the reference) that reaches it is the exception to the limit.
BIG_TILE_CASE = (8, 64, 64, 512, 512, 1, 1, 0)
EXACT_CONV_CASES = [
    ((2, 16, 24, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_conv_wgrad<64, 64>', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((1, 20, 12, 64, 128, 3, 2, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<64, 3, false>', 2: 'k_conv_wgrad<128, 64>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<64, 3, true>'}),
    ((3, 8, 8, 128, 128, 3, 1, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_conv_wgrad<128, 128>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((2, 12, 12, 64, 128, 1, 2, 0), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<64, 3, false>', 2: 'k_conv_wgrad<128, 64>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<64, 3, true>'}),
    ((1, 6, 10, 512, 128, 1, 1, 0), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_conv_wgrad<128, 128>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((2, 9, 7, 256, 256, 3, 1, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_conv_wgrad<128, 128>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((2, 32, 32, 64, 128, 3, 2, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<64, 2, false>', 2: 'k_conv_wgrad<128, 64>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<64, 2, true>'}),
    ((2, 32, 32, 64, 128, 1, 2, 0), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<64, 2, false>', 2: 'k_conv_wgrad<128, 64>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<64, 2, true>'}),
    ((2, 16, 32, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((1, 7, 96, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((3, 40, 64, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((2, 8, 32, 128, 128, 3, 1, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((1, 5, 64, 192, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((3, 16, 16, 128, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_wgrad3x3<16>', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((2, 6, 16, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3<16>', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((20, 4, 32, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((5, 12, 32, 64, 128, 3, 1, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((9, 1, 64, 64, 64, 3, 1, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<64, 0, false>', 2: 'k_wgrad3x3_ring2', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((1, 16, 16, 512, 512, 3, 1, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_wgrad3x3<16>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((2, 16, 16, 256, 512, 3, 2, 1), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 2, false>', 2: 'k_conv_wgrad<128, 128>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 2, true>'}),
    ((1, 17, 9, 128, 256, 1, 2, 0), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 3, false>', 2: 'k_conv_wgrad<128, 128>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 3, true>'}),
    ((2, 8, 8, 128, 128, 1, 1, 0), {}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>', 2: 'k_conv_wgrad<128, 128>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((2, 12, 12, 128, 64, 3, 2, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<128, 3, false>', 2: 'k_conv_wgrad<64, 128>', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<128, 3, true>'}),
    ((2, 16, 16, 128, 64, 3, 2, 1), {}, {0: 'k_conv_igemm<64, 0, false>', 1: 'k_conv_igemm<128, 2, false>', 2: 'k_conv_wgrad<64, 128>', 16: 'k_conv_igemm<64, 0, true>', 17: 'k_conv_igemm<128, 2, true>'}),
    ((2, 16, 32, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((2, 16, 32, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((1, 7, 96, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((1, 7, 96, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((3, 40, 64, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((3, 40, 64, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((2, 8, 32, 128, 128, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((2, 8, 32, 128, 128, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((1, 5, 64, 192, 64, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((1, 5, 64, 192, 64, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((20, 4, 32, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((20, 4, 32, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((5, 12, 32, 64, 128, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((5, 12, 32, 64, 128, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((9, 1, 64, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 0}, {2: 'k_wgrad3x3<32>'}),
    ((9, 1, 64, 64, 64, 3, 1, 1), {'wgrad_f32_ring': 1}, {2: 'k_wgrad3x3_ring'}),
    ((3, 16, 16, 64, 64, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch<64, false>', 1: 'k_conv3x3_patch<64, false>'}),
    ((3, 16, 16, 64, 64, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch<64, true>', 17: 'k_conv3x3_patch<64, true>'}),
    ((2, 32, 32, 128, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch<128, false>', 1: 'k_conv3x3_patch<128, false>'}),
    ((2, 32, 32, 128, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch<128, true>', 17: 'k_conv3x3_patch<128, true>'}),
    ((1, 64, 64, 64, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch<128, false>', 1: 'k_conv3x3_patch<64, false>'}),
    ((1, 64, 64, 64, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch<128, true>', 17: 'k_conv3x3_patch<64, true>'}),
    ((1, 8, 128, 64, 64, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch_roll<64, false>', 1: 'k_conv3x3_patch_roll<64, false>'}),
    ((1, 8, 128, 64, 64, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch_roll<64, true>', 17: 'k_conv3x3_patch_roll<64, true>'}),
    ((1, 4, 128, 128, 256, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch_roll<128, false>', 1: 'k_conv3x3_patch_roll<128, false>'}),
    ((1, 4, 128, 128, 256, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch_roll<128, true>', 17: 'k_conv3x3_patch_roll<128, true>'}),
    ((5, 16, 16, 256, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch<128, false>', 1: 'k_conv3x3_patch<128, false>'}),
    ((5, 16, 16, 256, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch<128, true>', 17: 'k_conv3x3_patch<128, true>'}),
    ((2, 6, 128, 128, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_patch_bn64': 1}, {0: 'k_conv3x3_patch_roll<128, false>', 1: 'k_conv3x3_patch_roll<128, false>'}),
    ((2, 6, 128, 128, 128, 3, 1, 1), {'conv_patch_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch_roll<128, true>', 17: 'k_conv3x3_patch_roll<128, true>'}),
    ((4, 16, 16, 256, 256, 3, 1, 1), {'conv_patch_min_tiles': 12, 'conv_patch_narrow': 1, 'conv_fwd_split_k': 0}, {0: 'k_conv3x3_patch<64, false>', 1: 'k_conv3x3_patch<64, false>', 16: 'k_conv_igemm<128, 0, true>', 17: 'k_conv_igemm<128, 0, true>'}),
    ((4, 16, 16, 256, 256, 3, 1, 1), {'conv_patch_min_tiles': 12, 'conv_patch_narrow': 0, 'conv_fwd_split_k': 0}, {0: 'k_conv_igemm<128, 0, false>', 1: 'k_conv_igemm<128, 0, false>'}),
    ((4, 16, 16, 256, 256, 3, 1, 1), {'conv_patch_min_tiles': 12, 'conv_patch_narrow': 2, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_patch<64, true>', 17: 'k_conv3x3_patch<64, true>'}),
    ((2, 16, 64, 64, 64, 3, 1, 1), {'conv_rows_f32_min_units': 1, 'conv_fwd_split_k': 0}, {0: 'k_conv3x3_c64_rows_f32', 1: 'k_conv3x3_c64_rows_f32'}),
    ((1, 21, 128, 64, 64, 3, 1, 1), {'conv_rows_f32_min_units': 1, 'conv_fwd_split_k': 0}, {0: 'k_conv3x3_c64_rows_f32', 1: 'k_conv3x3_c64_rows_f32'}),
    ((3, 9, 192, 64, 64, 3, 1, 1), {'conv_rows_f32_min_units': 1, 'conv_fwd_split_k': 0}, {0: 'k_conv3x3_c64_rows_f32', 1: 'k_conv3x3_c64_rows_f32'}),
    ((2, 40, 64, 64, 64, 3, 1, 1), {'conv_rows_f32_min_units': 1, 'conv_fwd_split_k': 0}, {0: 'k_conv3x3_c64_rows_f32', 1: 'k_conv3x3_c64_rows_f32'}),
    ((2, 16, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 1}, {16: 'k_conv3x3_c64_rows16_bf16', 17: 'k_conv3x3_c64_rows16_bf16'}),
    ((2, 16, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 0}, {16: 'k_conv3x3_c64_rows_bf16', 17: 'k_conv3x3_c64_rows_bf16'}),
    ((1, 24, 256, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 1}, {16: 'k_conv3x3_c64_rows16_bf16', 17: 'k_conv3x3_c64_rows16_bf16'}),
    ((1, 24, 256, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 0}, {16: 'k_conv3x3_c64_rows_bf16', 17: 'k_conv3x3_c64_rows_bf16'}),
    ((3, 9, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 1}, {16: 'k_conv3x3_c64_rows16_bf16', 17: 'k_conv3x3_c64_rows16_bf16'}),
    ((3, 9, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 0}, {16: 'k_conv3x3_c64_rows_bf16', 17: 'k_conv3x3_c64_rows_bf16'}),
    ((2, 1, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 1}, {16: 'k_conv3x3_c64_rows16_bf16', 17: 'k_conv3x3_c64_rows16_bf16'}),
    ((2, 1, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 0}, {16: 'k_conv3x3_c64_rows_bf16', 17: 'k_conv3x3_c64_rows_bf16'}),
    ((1, 2, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 1}, {16: 'k_conv3x3_c64_rows16_bf16', 17: 'k_conv3x3_c64_rows16_bf16'}),
    ((1, 2, 128, 64, 64, 3, 1, 1), {'conv_rows64_min_units': 1, 'conv_fwd_split_k': 0, 'conv_rows16': 0}, {16: 'k_conv3x3_c64_rows_bf16', 17: 'k_conv3x3_c64_rows_bf16'}),
    ((4, 32, 32, 128, 128, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_bf16_pp', 17: 'k_conv3x3_bf16_pp'}),
    ((2, 16, 16, 256, 256, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_bf16_pp', 17: 'k_conv3x3_bf16_pp'}),
    ((6, 16, 16, 128, 128, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_bf16_pp', 17: 'k_conv3x3_bf16_pp'}),
    ((1, 8, 128, 128, 128, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_bf16_pp', 17: 'k_conv3x3_bf16_pp'}),
    ((1, 8, 128, 128, 128, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_pp_strips': 0, 'conv_patch_min_tiles': 1}, {16: 'k_conv3x3_patch_roll<128, true>', 17: 'k_conv3x3_patch_roll<128, true>'}),
    ((1, 4, 256, 128, 128, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_bf16_pp', 17: 'k_conv3x3_bf16_pp'}),
    ((2, 12, 128, 128, 256, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0}, {16: 'k_conv3x3_bf16_pp', 17: 'k_conv3x3_bf16_pp'}),
    ((2, 12, 128, 128, 256, 3, 1, 1), {'conv_pp_min_tiles': 1, 'conv_fwd_split_k': 0, 'conv_pp_strips': 0, 'conv_patch_min_tiles': 1}, {16: 'k_conv3x3_patch_roll<128, true>', 17: 'k_conv3x3_patch_roll<128, true>'}),
    ((2, 16, 16, 64, 128, 1, 1, 0), {'conv1x1_stream_min_pixels': 32}, {16: 'k_conv1x1_stream_bf16<64, 2>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((1, 8, 20, 64, 128, 1, 1, 0), {'conv1x1_stream_min_pixels': 32}, {16: 'k_conv1x1_stream_bf16<64, 2>', 17: 'k_conv_igemm<64, 0, true>'}),
    ((3, 12, 8, 128, 128, 1, 1, 0), {'conv1x1_stream_min_pixels': 32}, {16: 'k_conv1x1_stream_bf16<128, 1>', 17: 'k_conv1x1_stream_bf16<128, 1>'}),
    ((2, 32, 32, 128, 128, 1, 1, 0), {'conv1x1_stream_min_pixels': 32}, {16: 'k_conv1x1_stream_bf16<128, 1>', 17: 'k_conv1x1_stream_bf16<128, 1>'}),
    ((8, 64, 64, 512, 512, 1, 1, 0), {}, {0: 'k_conv_igemm_big<128, 0, false>'}),
    ((8, 64, 64, 512, 512, 1, 1, 0), {'igemm_big_bf16': 1}, {16: 'k_conv_igemm_big<128, 0, true>'}),
    ((4, 128, 128, 256, 512, 1, 2, 0), {}, {1: 'k_conv_igemm_big<128, 2, false>'}),
    ((4, 128, 128, 256, 512, 1, 2, 0), {'igemm_big_bf16': 1}, {17: 'k_conv_igemm_big<128, 2, true>'}),
]

EXACT_SB_CASES = [  # sd_conv2d_fwd_sb: SB_CASES of tests/test_gpu_network.py
    (1, 128, 128, 64, 64, 3, 1, 1), (1, 64, 64, 128, 128, 3, 1, 1), (1, 32, 32, 256, 256, 3, 1, 1), (1, 16, 16, 512, 512, 3, 1, 1),
    (1, 128, 128, 64, 128, 3, 2, 1), (1, 128, 128, 64, 128, 1, 2, 0), (1, 16, 16, 512, 128, 1, 1, 0), (1, 32, 32, 256, 128, 1, 1, 0),
    (2, 9, 7, 256, 256, 3, 1, 1), (3, 20, 12, 64, 64, 3, 1, 1), (1, 24, 40, 64, 64, 5, 1, 2), (2, 32, 32, 64, 128, 7, 2, 3)]
EXACT_STEM_SHAPES = [(2, 64, 96), (5, 32, 32), (2, 136, 520)]
# sd_conv2d_wgrad_bf16: 3x3 / 1 ring forms (Wo % 32 == 0), the 16-wide form, k_wgrad_tap_bf16 (Cout % 128 == 0) and the widened fp32 path
EXACT_WGRAD_BF16_CASES = [(2, 32, 32, 64, 64, 3, 1, 1), (1, 16, 16, 128, 64, 3, 1, 1), (3, 32, 64, 64, 128, 3, 1, 1), (2, 20, 12, 64, 128, 3, 2, 1),
                          (4, 12, 12, 64, 128, 1, 2, 0), (2, 8, 8, 128, 128, 1, 1, 0), (1, 17, 9, 128, 256, 1, 2, 0), (20, 4, 32, 64, 64, 3, 1, 1),
                          (5, 12, 32, 64, 128, 3, 1, 1), (3, 7, 96, 128, 64, 3, 1, 1), (9, 1, 64, 64, 64, 3, 1, 1), (2, 12, 12, 128, 64, 3, 2, 1)]
WGRAD_BF16_RINGS = (0, 2, 3, 4, 5)
# statistics regime: (geometry, options, pass 0 / 16 kernel): tile kernels, ragged last tile, patch and row-stream epilogues
EXACT_STATS_CASES = [
    ((2, 16, 24, 64, 64, 3, 1, 1), {"conv_fwd_split_k": 0}, {0: "k_conv_igemm<64, 0, false>", 16: "k_conv_igemm<64, 0, true>"}),
    ((2, 9, 7, 256, 256, 3, 1, 1), {"conv_fwd_split_k": 0}, {0: "k_conv_igemm<128, 0, false>", 16: "k_conv_igemm<128, 0, true>"}),
    ((1, 16, 16, 512, 512, 3, 1, 1), {}, {0: "k_conv_igemm<128, 0, false>", 16: "k_conv_igemm<128, 0, true>"}),      # split-K: two-pass form
    ((2, 12, 12, 64, 128, 1, 2, 0), {"conv_fwd_split_k": 0}, {0: "k_conv_igemm<128, 0, false>", 16: "k_conv_igemm<128, 0, true>"}),
    ((2, 32, 32, 128, 128, 3, 1, 1), {"conv_patch_min_tiles": 1, "conv_fwd_split_k": 0}, {0: "k_conv3x3_patch<128, false>", 16: "k_conv3x3_patch<128, true>"}),
    ((1, 8, 128, 64, 64, 3, 1, 1), {"conv_patch_min_tiles": 1, "conv_fwd_split_k": 0, "conv_patch_bn64": 1},
     {0: "k_conv3x3_patch_roll<64, false>", 16: "k_conv3x3_patch_roll<64, true>"}),
    ((3, 9, 192, 64, 64, 3, 1, 1), {"conv_rows_f32_min_units": 1, "conv_fwd_split_k": 0}, {0: "k_conv3x3_c64_rows_f32"}),
    ((3, 9, 128, 64, 64, 3, 1, 1), {"conv_rows64_min_units": 1, "conv_fwd_split_k": 0, "conv_rows16": 0}, {16: "k_conv3x3_c64_rows_bf16"}),
    ((4, 32, 32, 128, 128, 3, 1, 1), {"conv_pp_min_tiles": 1, "conv_fwd_split_k": 0}, {16: "k_conv3x3_bf16_pp"}),
]
# sd_conv2d_dgrad_bn_reduce_sums: (geometry, options, pass 1 kernel)
EXACT_BNRED_CASES = [
    ((2, 16, 24, 64, 64, 3, 1, 1), {}, "k_conv_igemm<64, 0, false>"),
    ((2, 9, 7, 256, 256, 3, 1, 1), {}, "k_conv_igemm<128, 0, false>"),
    ((2, 32, 32, 64, 128, 3, 2, 1), {}, "k_conv_igemm<64, 2, false>"),
    ((2, 32, 32, 128, 128, 3, 1, 1), {"conv_patch_min_tiles": 1}, "k_conv3x3_patch<128, false>"),
    ((1, 8, 128, 64, 64, 3, 1, 1), {"conv_patch_min_tiles": 1, "conv_patch_bn64": 1}, "k_conv3x3_patch_roll<64, false>"),
]
# heads (B, H, W, C, Co): generic path (HW % 16 != 0, C != 128, 16 < Co <= 32), the C = 128 / Co <= 16 MFMA path, the wide path (Co > 32:
# one Co that is no multiple of 16 and one that is; ragged pixel tiles)
EXACT_HEAD_CASES = [(2, 6, 10, 128, 7), (2, 16, 16, 64, 5), (1, 12, 12, 128, 20), (2, 48, 48, 128, 7), (3, 16, 20, 128, 16),
                    (2, 24, 24, 128, 33), (1, 45, 37, 64, 100), (2, 16, 16, 256, 64)]
EXACT_HEAD_BF16_BWD_CASES = [(2, 6, 10, 128, 7), (3, 32, 40, 128, 8), (2, 16, 16, 64, 5)]
# fused FPN conv + head (k_conv3x3_bf16_pp_head): (B, H, W, Cin, head channels)
EXACT_FUSED_HEAD_CASES = [(4, 32, 32, 128, 7), (1, 8, 128, 128, 20), (2, 16, 16, 256, 32)]


def case_id(entry):
    geom, opts = entry[0], entry[1]
    return "x".join(str(v) for v in geom) + "".join(f"-{k.replace('conv_', '')}{v}" for k, v in opts.items())


# -- operand regimes: seeded generators of integer-valued fp32 tensors -----------------------------
def int_uniform(g, shape, a):
    import torch
    return torch.randint(-a, a + 1, tuple(shape), generator=g).float()


def half_integers(g, shape, a):
    """multiples of 0.5 in [-a, a]"""
    import torch
    return torch.randint(-2 * a, 2 * a + 1, tuple(shape), generator=g).float() / 2


def pow2_scales(g, n):
    import torch
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]


def ternary(g, shape, density):
    import torch
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    return sign * (torch.rand(tuple(shape), generator=g) < density).float()


# amplitude pairs of the rounding regime, widest first: integers up to 15 are exact in bf16
_AMPLITUDES = [(15, 15), (15, 11), (15, 7), (11, 7), (8, 6), (8, 4), (6, 4), (4, 4), (4, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1)]


def rounding_amplitudes(K, target=900.0):
    """Amplitudes (a, b) of the two operands of a K-term reduction whose sums have a standard deviation near `target`: a uniform integer in
    [-a, a] has variance a (a + 1) / 3.  Around 900 the outputs straddle the bf16 binades with an ulp of 2 .. 16 (256 .. 4096), where an
    integer needs rounding with probability 1 - 1/ulp and is a tie with probability 1/ulp; much larger sums have almost no ties, much smaller
    ones need no rounding (the [-3, 3] x [-2, 2] range of a 576-term conv rounds nothing)."""
    import math
    best = min(_AMPLITUDES, key=lambda ab: abs(math.log(math.sqrt(K * ab[0] * (ab[0] + 1) * ab[1] * (ab[1] + 1) / 9.0) / target)))
    return best


def rounding_pair(g, shape_a, shape_b, K):
    a, b = rounding_amplitudes(K)
    return int_uniform(g, shape_a, a), int_uniform(g, shape_b, b)


def wide_pair(g, shape_a, shape_b, K, wide_first):
    """one operand with 12 significant bits (integers in [-2047, 2047]), the other in {-1, 0, 1}, thinned so that a K-term sum of absolute
    products stays near 3000 * 1024 (below 2^22)"""
    density = min(2.0 / 3.0, 3000.0 / K)
    if wide_first:
        return int_uniform(g, shape_a, 2047), ternary(g, shape_b, density)
    return ternary(g, shape_a, density), int_uniform(g, shape_b, 2047)


def stats_pair(g, shape_a, shape_b, K, pixels):
    """statistics regime: the widest of the small ranges for which pixels * E[y^2] = pixels * K * var(a) * var(b) stays below 2^22 (the
    asserted bound is on the actual sums)"""
    for a, b in ((3, 2), (2, 2), (2, 1), (1, 1)):
        if pixels * K * (a * (a + 1) / 3.0) * (b * (b + 1) / 3.0) < 2 ** 22:
            break
    return int_uniform(g, shape_a, a), int_uniform(g, shape_b, b)


# -- bf16 rounding on fp32 bit patterns (independent of torch's conversion) ---------------------------
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(b):
    import torch
    b = b & 0xFFFFFFFF
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32)


def bf16_rne(t32):
    """fp32 tensor -> fp32 tensor holding round-to-nearest-even bf16 values (finite inputs)"""
    b = _bits(t32)
    return _from_bits((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000)


def bf16_trunc(t32):
    return _from_bits(_bits(t32) & 0xFFFF0000)


def rounding_shares(ref32):
    """(share not representable in bf16, share of exact ties, share where truncation differs from nearest-even)"""
    low = _bits(ref32) & 0xFFFF
    return (float((low != 0).double().mean()), float((low == 0x8000).double().mean()),
            float((bf16_rne(ref32) != bf16_trunc(ref32)).double().mean()))


ROUNDING_SHARES_MIN = (0.20, 0.05, 0.05)


def assert_rounding_coverage(ref32, what=""):
    s = rounding_shares(ref32)
    assert all(v >= m for v, m in zip(s, ROUNDING_SHARES_MIN)), f"{what}: inexact / ties / truncation-differs shares {s} below {ROUNDING_SHARES_MIN}"
    return s


# -- fp64 references and their worst-case bounds ------------------------------------------------------
def conv_ref(x, w, stride, pad):
    import torch.nn.functional as F
    return F.conv2d(x.double(), w.double(), None, stride, pad)


def dgrad_ref(dy, w, x_shape, stride, pad):
    import torch
    return torch.nn.grad.conv2d_input(tuple(x_shape), w.double(), dy.double(), stride, pad)


def wgrad_ref(dy, x, w_shape, stride, pad):
    import torch
    return torch.nn.grad.conv2d_weight(x.double(), tuple(w_shape), dy.double(), stride, pad)


def epilogue_ref(conv64, scale=None, shift=None, res=None, relu=False):
    y = conv64
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0) if relu else y


def assert_exact_reference(ref64, bound64, limit=EXACT_LIMIT, what=""):
    """the conditions on the inputs: worst-case bound below the limit everywhere, and the fp64 reference equal to its own fp32 rounding"""
    import torch
    assert float(bound64.max()) < limit, f"{what}: worst-case bound {float(bound64.max()):.0f} >= {limit:.0f}"
    assert float(ref64.abs().max()) <= float(bound64.max())
    assert torch.equal(ref64.float().double(), ref64), f"{what}: the reference is not exact in fp32"
    return ref64.float()


def assert_equal_report(got, ref, what="", layout="bhwc"):
    """torch.equal with a report: count of mismatches and the first few with their position (named by `layout`) and both values.
    NaN in `got` (an element the kernel never wrote) is a mismatch."""
    import torch
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()
    lines = [f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (shape {tuple(got.shape)}, position = {layout})"]
    for i in idx[:8].tolist():
        lines.append(f"  {tuple(i)}: got {float(got[tuple(i)])!r}, want {float(ref[tuple(i)])!r}")
    raise AssertionError("\n".join(lines))


# -- the problems the CPU and the GPU module share (cached: a reference is computed once and never modified) --------
def _seed(geom, salt):
    return (sum((i + 3) * 7919 * int(v) for i, v in enumerate(geom)) + 104729 * salt) % (2 ** 31)


def _pair(g, regime, shape_a, shape_b, K, pixels):
    if regime == "round":
        return rounding_pair(g, shape_a, shape_b, K)
    if regime == "stats":
        return stats_pair(g, shape_a, shape_b, K, pixels)
    return wide_pair(g, shape_a, shape_b, K, regime == "wide_a")


import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def fwd_problem(geom, regime="round"):
    """x (B, Cin, H, W), w (Cout, Cin, k, k) and the fp64 conv with its worst-case bound conv(|x|, |w|); regime: round / wide_a (x wide) /
    wide_b (w wide) / stats"""
    import torch
    B, H, W, cin, cout, k, stride, pad = geom
    g = torch.Generator().manual_seed(_seed(geom, {"round": 1, "wide_a": 2, "wide_b": 3, "stats": 4}[regime]))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x, w = _pair(g, regime, (B, cin, H, W), (cout, cin, k, k), cin * k * k, B * Ho * Wo)
    ref, bound = conv_ref(x, w, stride, pad), conv_ref(x.abs(), w.abs(), stride, pad)
    return {"x": x, "w": w, "ref": ref, "bound": bound}


@functools.lru_cache(maxsize=None)
def dgrad_problem(geom, regime="round"):
    """dy (B, Cout, Ho, Wo), w and the fp64 data gradient with its bound; wide_a: dy wide, wide_b: w wide"""
    import torch
    B, H, W, cin, cout, k, stride, pad = geom
    g = torch.Generator().manual_seed(_seed(geom, {"round": 5, "wide_a": 6, "wide_b": 7, "stats": 8}[regime]))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    K = cout * (-(-k // stride)) ** 2                    # taps that reach one input pixel
    dy, w = _pair(g, regime, (B, cout, Ho, Wo), (cout, cin, k, k), K, B * H * W)
    ref = dgrad_ref(dy, w, (B, cin, H, W), stride, pad)
    bound = dgrad_ref(dy.abs(), w.abs(), (B, cin, H, W), stride, pad)
    return {"dy": dy, "w": w, "ref": ref, "bound": bound}


@functools.lru_cache(maxsize=None)
def wgrad_problem(geom, regime="round"):
    """dy, x and the fp64 weight gradient (Cout, Cin, k, k) with its bound sum |dy| |x|; wide_a: dy wide, wide_b: x wide"""
    import torch
    B, H, W, cin, cout, k, stride, pad = geom
    g = torch.Generator().manual_seed(_seed(geom, {"round": 9, "wide_a": 10, "wide_b": 11}[regime]))
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if regime == "round":      # no bf16 output here: the widest bf16-exact integers the pixel count allows
        a = 15 if B * Ho * Wo * 225 < EXACT_LIMIT else 8
        dy, x = int_uniform(g, (B, cout, Ho, Wo), a), int_uniform(g, (B, cin, H, W), a)
    else:
        dy, x = wide_pair(g, (B, cout, Ho, Wo), (B, cin, H, W), B * Ho * Wo, regime == "wide_a")
    ref = wgrad_ref(dy, x, (cout, cin, k, k), stride, pad)
    bound = wgrad_ref(dy.abs(), x.abs(), (cout, cin, k, k), stride, pad)
    return {"dy": dy, "x": x, "ref": ref, "bound": bound}


def epilogue_operands(geom_or_seed, channels, res_shape, salt=0, wide=False):
    """scale in {0.5, 1, 2}, half-integer shift, integer residual (12 significant bits in the wide regime)"""
    import torch
    g = torch.Generator().manual_seed(_seed(tuple(geom_or_seed), 20 + salt))
    return pow2_scales(g, channels), half_integers(g, (channels,), 32), int_uniform(g, res_shape, 2047 if wide else 63)


def epilogue_bound(bound64, scale=None, shift=None, res=None):
    b = bound64
    if scale is not None:
        b = b * scale.double().abs().view(1, -1, 1, 1)
    if shift is not None:
        b = b + shift.double().abs().view(1, -1, 1, 1)
    if res is not None:
        b = b + res.double().abs()
    return b


@functools.lru_cache(maxsize=None)
def stem_problem(shape, regime="round"):
    """image (B, 3, H, W), weights (64, 3, 7, 7), fp64 conv 7x7 / 2 / 3 and its bound"""
    B, H, W = shape
    return fwd_problem((B, H, W, 3, 64, 7, 2, 3), regime)


@functools.lru_cache(maxsize=None)
def head_problem(case, regime="round"):
    """x (B, C, H, W), w (Co, C), bias (Co), dy (B, Co, H, W) integers; fp64 forward, dx, dw, dbias and their bounds"""
    import torch
    B, H, W, Cc, Co = case
    g = torch.Generator().manual_seed(_seed(case, {"round": 12, "wide_a": 13, "wide_b": 14}[regime]))
    if regime == "round":
        x, w = int_uniform(g, (B, Cc, H, W), 15), int_uniform(g, (Co, Cc), 63)      # (w is fp32 on every path; |w| <= 256 is exact in bf16 too)
        dy = int_uniform(g, (B, Co, H, W), 15 if B * H * W * 225 < EXACT_LIMIT else 8)
    else:
        x, w = wide_pair(g, (B, Cc, H, W), (Co, Cc), Cc, regime == "wide_a")
        dy = ternary(g, (B, Co, H, W), min(2.0 / 3.0, 3000.0 / (B * H * W)))
    bias = int_uniform(g, (Co,), 63)
    xd, wd, dyd = x.double(), w.double(), dy.double()
    out = {"x": x, "w": w, "bias": bias, "dy": dy,
           "y": torch.einsum("bchw,oc->bohw", xd, wd) + bias.double().view(1, -1, 1, 1),
           "y_bound": torch.einsum("bchw,oc->bohw", xd.abs(), wd.abs()) + bias.double().abs().view(1, -1, 1, 1),
           "dx": torch.einsum("bohw,oc->bchw", dyd, wd), "dx_bound": torch.einsum("bohw,oc->bchw", dyd.abs(), wd.abs()),
           "dw": torch.einsum("bohw,bchw->oc", dyd, xd), "dw_bound": torch.einsum("bohw,bchw->oc", dyd.abs(), xd.abs()),
           "db": dyd.sum((0, 2, 3)), "db_bound": dyd.abs().sum((0, 2, 3))}
    return out


# ---------------------------------------------------------------------------------------------
# the legacy preprocess entry points of the C API, called by name with positional arguments
# ---------------------------------------------------------------------------------------------
def call_legacy_preprocess_form(fn_name, source, B, Hin, Win, out_size, flips, mean, std, jitter, affine, mosaic, window, letterbox, blur, dev,
                                persp=None, jpeg=None, tone=None, noise=None):
    """Calls the legacy entry point `fn_name` (`sd_preprocess_images[_list][_jitter | _affine | _mosaic | _window | _letterbox | _blur |
    _persp | _jpeg | _tone | _noise]`) the way a C caller does: positional arguments in the order of include/sdnet_hip.h and a workspace of
    the form's own size query.  source = the address of the packed images or of the pointer table; the tables are those data/augment.py
    uploads for the same arguments.  A stage the form has no argument for must be None."""
    from structuredetector_amd import _lib as L
    from structuredetector_amd.data.augment import _chain_desc
    lib = L.lib()
    form = fn_name.replace("sd_preprocess_images", "").replace("_list", "").lstrip("_")      # "" = the plain resize
    forms = ["", "jitter", "affine", "mosaic", "window", "letterbox", "blur", "persp", "jpeg", "tone", "noise"]
    late = forms.index(form) - forms.index("blur")                                          # >= 0: the forms that take a geometry
    d, out, keep = _chain_desc(source, "_list" in fn_name, B, Hin, Win, out_size, flips, mean, std, jitter, affine, mosaic, window, letterbox, blur,
                               persp, jpeg, tone, noise, dev)
    given = dict(jitter=jitter, affine=affine, mosaic=mosaic, window=window, letterbox=letterbox, blur=blur, persp=persp, jpeg=jpeg, tone=tone,
                 noise=noise)
    takes = {"": (), "jitter": ("jitter",), "affine": ("jitter", "affine"), "mosaic": ("jitter", "affine", "mosaic"),
             "window": ("jitter", "affine", "mosaic", "window"), "letterbox": ("jitter", "affine", "mosaic", "letterbox")}
    takes = takes.get(form, ("jitter", "affine", "mosaic", "window", "letterbox") + tuple(forms[6:7 + max(late, 0)]))
    assert all(v is None or k in takes for k, v in given.items()), f"{fn_name} has no argument for {[k for k, v in given.items() if v is not None]}"
    tables = [d.h_bounds, d.h_kk, d.h_ksize, d.v_bounds, d.v_kk, d.v_ksize]
    jit, mos, end = [d.jitter_order, d.jitter_factors], [d.mosaic_geom, d.mosaic_affine], [d.mean3, d.std3, d.out]
    if late >= 0:
        args = [source, d.geometry, B, Hin, Win, d.Hg, d.Wg, d.Hout, d.Wout, d.g0, d.g1, *tables, d.window, d.flips, *jit, d.affine]
        args += ([d.persp] if late >= 1 else []) + mos + [d.blur] + [d.jpeg, d.tone, d.noise][:max(late - 1, 0)] + [d.fill3]
        size = {0: lib.sd_preprocess_blur_workspace_bytes, 1: lib.sd_preprocess_blur_workspace_bytes, 2: lib.sd_preprocess_jpeg_workspace_bytes,
                3: lib.sd_preprocess_tone_workspace_bytes, 4: lib.sd_preprocess_noise_workspace_bytes}[late]
        nbytes = size(d.geometry, B, Hin, Win, d.Wg, d.Hout, d.Wout, d.g0)
    elif form == "window":
        args = [source, B, Hin, Win, d.Hg, d.Wg, d.Hout, d.Wout, *tables, d.window, d.g0, d.g1, d.flips, *jit, d.affine, *mos, d.fill3]
        nbytes = lib.sd_preprocess_window_workspace_bytes(B, d.g0, d.Hout, d.Wout)
    elif form == "letterbox":
        args = [source, B, Hin, Win, d.Hg, d.Wg, d.Hout, d.Wout, d.g0, d.g1, *tables, d.flips, *jit, d.affine, *mos, d.fill3]
        nbytes = lib.sd_preprocess_letterbox_workspace_bytes(B, Hin, d.Wg, d.Hout, d.Wout)
    else:
        stages = {"": [], "jitter": jit, "affine": jit + [d.affine, d.fill3], "mosaic": jit + [d.affine] + mos + [d.fill3]}[form]
        args = [source, B, Hin, Win, d.Hout, d.Wout, *tables, d.flips, *stages]
        nbytes = (lib.sd_preprocess_workspace_bytes(B, Hin, Win, d.Wout) if form == "" else
                  getattr(lib, f"sd_preprocess_{form}_workspace_bytes")(B, Hin, Win, d.Hout, d.Wout))
    ws = L.workspace(nbytes, dev)
    L.check(getattr(lib, fn_name)(*args, *end, ws.data_ptr(), ws.numel(), L.stream()), fn_name)
    del keep
    return out


# ---------------------------------------------------------------------------------------------
# launch trace of the network engine (tests/test_gpu_engine_trace.py, tools/engine_trace.py)
# ---------------------------------------------------------------------------------------------
def _trace_arg(a):
    """A `byref(struct)` as the struct's field tuple, a float as itself, an int below 2^20 as itself, anything else as 0 / "p" (null or not)."""
    obj = getattr(a, "_obj", None)
    if obj is not None and hasattr(obj, "_fields_"):
        return tuple(getattr(obj, f) for f, _ in obj._fields_)
    if isinstance(a, float):
        return a
    if isinstance(a, int):
        return int(a) if a < 2 ** 20 else "p"
    return "p" if a else 0


class LaunchRecorder:
    """Stand-in for `_Engine.lib`: every attribute is the real library's function behind a wrapper that first notes
    (symbol, canonical arguments) in `calls`.  Entry point, geometry, flags, modes, the null-ness of every buffer and the order."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, tuple(_trace_arg(a) for a in args)))
            return fn(*args)
        self.__dict__[name] = call
        return call

    def lines(self):
        return [f"{name}({', '.join(repr(a) for a in args)})" for name, args in self.calls]
