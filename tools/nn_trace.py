#!/usr/bin/env python3
"""Call trace of the BatchNorm / pool / head / optimizer host layer (the tail of structuredetector_amd/csrc/sd_nn.hip): every entry point
once per case, on inputs made on the CPU from fixed seeds.  Per call: the return code (and the error text of a refusal), the first 12 hex
digits of the SHA-256 of every output buffer and of the workspace, and the answers of the size queries.

  run [--out FILE]                    the calls of this checkout's library as JSON (digests only: no launch sequences)
  run --sep [--out FILE]              the same with one separator kernel in front of every call, for a run under
                                      `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/nn_trace.py run --sep`
  launches CSV [--out FILE]           the per-call launch sequences of such a run, read from its *_kernel_trace.csv
  fixture RUN.json LAUNCHES.json      tests/golden/nn_call_trace.json from the two (record it on the commit the code under test must
                                      equal, never on that code)

A call's record also carries `desc`, the fields (DESC_FIELDS) of the sd_nn_call_desc that asks sd_nn_kernel_names for the same call
(tests/test_nn_plan_cpu.py).  Cases: tests/bn_ref.py SHAPES and ROW_CASES, the shape tables of tests/pool_ref.py, the head cases of
tests/helpers.py -- the smallest shape per dispatch branch that the suite names, nothing larger."""
import argparse
import csv
import hashlib
import json
import re
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE))
FIXTURE = HERE / "tests" / "golden" / "nn_call_trace.json"

# sd_nn_call_desc.op (include/sdnet_hip.h)
OPS = ("bn_train_stats", "bn_finalize_stats", "bn_stats_from_sums", "bn_apply", "bn_fold", "bn_bwd", "bn_bwd_reduce", "bn_bwd_finalize",
       "bn_bwd_means_from_sums", "bn_bwd_apply", "col_sum", "maxpool_fwd", "maxpool_bwd", "bn_relu_maxpool_fwd", "stem_bwd", "stem_bwd_reduce",
       "stem_bwd_apply", "upsample_bwd", "cast", "head_fwd", "head_bwd", "adam", "grad_sumsq", "optim")
F_SCRATCH, F_SUMS, F_DECAY, F_CLIP, F_EMA = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12      # bits 0..3: pointer slot k is 16-byte aligned
ALL_ALIGNED = 15
DIGEST_HEX = 12                                      # hex digits kept of every SHA-256


DESC_FIELDS = ("op", "form", "B", "H", "W", "M", "C", "Co", "relu", "rows", "flags", "pool_fwd_pair")      # sd_nn_call_desc, in order


def desc(op, form=0, B=0, H=0, W=0, M=0, C=0, Co=0, relu=0, rows=0, flags=ALL_ALIGNED, pair=1):
    return [OPS.index(op), form, B, H, W, M, C, Co, relu, rows, flags, pair]


class Recorder:
    def __init__(self, sep):
        import torch

        from structuredetector_amd import _lib as L
        self.torch, self.L, self.lib, self.dev = torch, L, L.lib(), torch.device("cuda")
        self.sep = torch.zeros(64, dtype=torch.int32, device=self.dev) if sep else None
        self.calls = []
        if sep:
            self.sep.bitwise_not_()                # the separator: the one bitwise_not kernel of the process
            torch.cuda.synchronize()

    def up(self, t, bf16=False, offset=False):
        """CPU tensor -> device (bf16: rounded; offset: the data pointer 8 bytes past a 16-byte boundary)."""
        torch = self.torch
        t = t.contiguous()
        if bf16:
            t = t.bfloat16()
        if not offset:
            return t.to(self.dev)
        pad = 8 // t.element_size()
        buf = torch.empty(t.numel() + pad, dtype=t.dtype, device=self.dev)
        view = buf[pad:].view(t.shape)
        view.copy_(t)
        return view

    def out(self, shape, dtype=None, offset=False, like=None):
        """A device buffer the call writes, pre-filled so that bytes the call leaves alone hash the same every time."""
        torch = self.torch
        dtype = dtype or torch.float32
        src = torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), 3, dtype=dtype) if like is None else like.clone().to(dtype)
        return self.up(src, offset=offset)

    def ws(self, nbytes):
        return self.torch.full((max(int(nbytes), 256),), 0xA5, dtype=self.torch.uint8, device=self.dev)

    def call(self, name, d, fn, outs, sizes=None):
        torch = self.torch
        torch.cuda.synchronize()
        if self.sep is not None:
            self.sep.bitwise_not_()
        rc = fn()
        torch.cuda.synchronize()
        rec = {"name": name, "desc": d, "rc": rc}
        if rc:
            rec["error"] = self.lib.sd_last_error().decode(errors="replace")
        else:
            rec["out"] = {k: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:DIGEST_HEX]
                          for k, t in outs.items()}
        if sizes:
            rec["sizes"] = sizes
        self.calls.append(rec)


def p(t):
    return None if t is None else t.data_ptr()


def run_calls(sep=False):
    import torch

    from tests import bn_ref as R
    from tests import helpers as X
    from tests import pool_ref as P
    r = Recorder(sep)
    lib, L = r.lib, r.L
    st = L.stream()
    gen = lambda seed: torch.Generator().manual_seed(seed)
    ints = lambda g, shape, a: torch.randint(-a, a + 1, shape, generator=g).float()

    # ---- BatchNorm and column sums over [M][C] --------------------------------------------------------------------------------------------
    for k, (tag, (M, C)) in enumerate(R.SHAPES.items()):
        g = gen(k)
        q = R.exact_params(C)
        x, dy, y1 = ints(g, (M, C), 3), ints(g, (M, C), 4), ints(g, (M, C), 2)
        mask = torch.randint(0, 16, (M * C // 4,), generator=g).to(torch.uint8)
        nws = lib.sd_col_reduce_workspace_bytes(M, C)
        sizes = {"col_reduce_workspace_bytes": nws}
        par = {n: r.up(getattr(q, n)) for n in ("mean", "invstd", "gamma", "beta", "mg", "mgx", "prior0", "prior1")}
        means = r.up(torch.cat([q.mg, q.mgx]))
        maskd = r.up(mask)
        # the smallest shape takes every relu x accumulate (the split forms every relu), the others one pair each
        combos = [(relu, acc) for relu in range(4) for acc in range(2)] if k == 0 else [(k % 4, k % 2)]
        for form in (0, 1):
            sfx, bf = ("", False) if form == 0 else ("_bf16", True)
            for off in ((False,) if form == 0 else (False, True)):
                al = 0 if off else ALL_ALIGNED
                otag = f"{tag}{sfx}{'_off8' if off else ''}"
                xd, dyd, yd = r.up(x, bf, off), r.up(dy, bf, off), r.up(y1, bf, off)
                odt = torch.bfloat16 if bf else torch.float32
                if not off:
                    mean, invstd, rm, rv, ws = r.out(C), r.out(C), r.out(C, like=q.prior0), r.out(C, like=q.prior1), r.ws(nws)
                    fn = getattr(lib, "sd_bn_train_stats" + sfx)
                    r.call(f"bn_train_stats{sfx}/{tag}", desc("bn_train_stats", form, M=M, C=C),
                           lambda: fn(p(xd), M, C, R.EPS, R.MOMENTUM, p(rm), p(rv), p(mean), p(invstd), p(ws), nws, st),
                           dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv, ws=ws), sizes)
                    sums, ws = r.out(2 * C + 1, torch.float64), r.ws(nws)
                    fn = getattr(lib, "sd_bn_train_sums" + sfx)
                    r.call(f"bn_train_sums{sfx}/{tag}", desc("bn_train_stats", form, M=M, C=C, flags=ALL_ALIGNED | F_SUMS),
                           lambda: fn(p(xd), M, C, p(sums), p(ws), nws, st), dict(sums=sums, ws=ws))
                    for acc in ((0, 1) if k == 0 else (k % 2,)):
                        o, ws = r.out(C, like=q.prior0), r.ws(nws)
                        fn = getattr(lib, "sd_col_sum" + sfx)
                        r.call(f"col_sum{sfx}/{tag}/acc{acc}", desc("col_sum", form, M=M, C=C),
                               lambda: fn(p(xd), M, C, p(o), acc, p(ws), nws, st), dict(out=o, ws=ws))
                # apply: plain, and residual + ReLU + mask bytes
                for res, relu in ((None, 0), (r.up(dy, bf, off), 1)):
                    yo, mo = r.out((M, C), odt, off), r.out(M * C // 4, torch.uint8)
                    fn = getattr(lib, "sd_bn_apply" + sfx)
                    r.call(f"bn_apply{sfx}/{otag}/relu{relu}", desc("bn_apply", form, M=M, C=C, relu=relu, flags=al),
                           lambda: fn(p(xd), p(yo), M, C, p(par["mean"]), p(par["invstd"]), p(par["gamma"]), p(par["beta"]), p(res), relu,
                                      p(mo) if relu else None, st), dict(y=yo, mask=mo))
                for relu, acc in combos:
                    yarg = yd if relu == 1 else maskd if relu == 3 else None
                    dx, go, dg, db, ws = r.out((M, C), odt, off), r.out((M, C), odt, off), r.out(C, like=q.prior0), r.out(C, like=q.prior1), r.ws(nws)
                    fn = getattr(lib, "sd_bn_bwd" + sfx)
                    r.call(f"bn_bwd{sfx}/{otag}/relu{relu}/acc{acc}", desc("bn_bwd", form, M=M, C=C, relu=relu, flags=al),
                           lambda: fn(p(dyd), p(xd), p(yarg), relu, M, C, p(par["mean"]), p(par["invstd"]), p(par["gamma"]), p(par["beta"]), p(dx),
                                      p(go), p(dg), p(db), acc, p(ws), nws, st), dict(dx=dx, g_out=go, dgamma=dg, dbeta=db, ws=ws))
                    if k == 0 and acc != relu % 2:
                        continue
                    dg, db, sums, ws = r.out(C, like=q.prior0), r.out(C, like=q.prior1), r.out(2 * C + 1, torch.float64), r.ws(nws)
                    fn = getattr(lib, "sd_bn_bwd_reduce" + sfx)
                    r.call(f"bn_bwd_reduce{sfx}/{otag}/relu{relu}/acc{acc}", desc("bn_bwd_reduce", form, M=M, C=C, relu=relu, flags=al | F_SUMS),
                           lambda: fn(p(dyd), p(xd), p(yarg), relu, M, C, p(par["mean"]), p(par["invstd"]), p(par["gamma"]), p(par["beta"]),
                                      p(dg), p(db), acc, p(sums), p(ws), nws, st), dict(dgamma=dg, dbeta=db, sums=sums, ws=ws))
                    dx, go = r.out((M, C), odt, off), r.out((M, C), odt, off)
                    fn = getattr(lib, "sd_bn_bwd_apply" + sfx)
                    r.call(f"bn_bwd_apply{sfx}/{otag}/relu{relu}", desc("bn_bwd_apply", form, M=M, C=C, relu=relu, flags=al),
                           lambda: fn(p(dyd), p(xd), p(yarg), relu, M, C, p(par["mean"]), p(par["invstd"]), p(par["gamma"]), p(par["beta"]),
                                      p(means), p(dx), p(go), st), dict(dx=dx, g_out=go))

    # ---- the finish kernels on caller-provided partial rows ---------------------------------------------------------------------------------
    for k, (tag, (rows, C)) in enumerate(R.ROW_CASES.items()):
        g = gen(100 + k)
        q = R.exact_params(C)
        M = rows * 16
        part = r.up(ints(g, (rows, 2, C), 5))
        srows = lib.sd_bn_finalize_scratch_rows(rows)
        sizes = {"bn_finalize_scratch_rows": srows}
        for with_scratch in (1, 0):
            fl = ALL_ALIGNED | (F_SCRATCH if with_scratch else 0)
            nm = f"{tag}/scratch{with_scratch}"
            new_scratch = lambda: r.out(max(srows, 1) * 2 * C) if with_scratch else None
            mean, invstd, rm, rv, sc = r.out(C), r.out(C), r.out(C, like=q.prior0), r.out(C, like=q.prior1), new_scratch()
            outs = dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv)
            r.call(f"bn_finalize_stats/{nm}", desc("bn_finalize_stats", M=M, C=C, rows=rows, flags=fl),
                   lambda: lib.sd_bn_finalize_stats(p(part), rows, M, C, R.EPS, R.MOMENTUM, p(rm), p(rv), p(mean), p(invstd), p(sc), st),
                   dict(outs, scratch=sc) if with_scratch else outs, sizes)
            sums, sc = r.out(2 * C + 1, torch.float64), new_scratch()
            r.call(f"bn_stats_sums/{nm}", desc("bn_finalize_stats", M=M, C=C, rows=rows, flags=fl | F_SUMS),
                   lambda: lib.sd_bn_stats_sums(p(part), rows, M, C, p(sums), p(sc), st), dict(sums=sums))
            acc = (k + with_scratch) % 2
            dg, db, mo, sc = r.out(C, like=q.prior0), r.out(C, like=q.prior1), r.out(2 * C), new_scratch()
            r.call(f"bn_bwd_finalize/{nm}/acc{acc}", desc("bn_bwd_finalize", M=M, C=C, rows=rows, flags=fl),
                   lambda: lib.sd_bn_bwd_finalize(p(part), rows, M, C, p(dg), p(db), acc, p(mo), p(sc), st), dict(dgamma=dg, dbeta=db, means=mo))
            dg, db, sums, sc = r.out(C, like=q.prior0), r.out(C, like=q.prior1), r.out(2 * C + 1, torch.float64), new_scratch()
            r.call(f"bn_bwd_sums/{nm}/acc{acc}", desc("bn_bwd_finalize", M=M, C=C, rows=rows, flags=fl | F_SUMS),
                   lambda: lib.sd_bn_bwd_sums(p(part), rows, M, C, p(dg), p(db), acc, p(sums), p(sc), st), dict(dgamma=dg, dbeta=db, sums=sums))
    for C in (4, 64, 1024):
        g = gen(200 + C)
        q = R.exact_params(C)
        sums = r.up(torch.cat([ints(g, (C,), 50).double(), (ints(g, (C,), 50).double().abs() + 60) * 8, torch.tensor([64.0], dtype=torch.float64)]))
        mean, invstd, rm, rv, mo = r.out(C), r.out(C), r.out(C, like=q.prior0), r.out(C, like=q.prior1), r.out(2 * C)
        r.call(f"bn_stats_from_sums/C{C}", desc("bn_stats_from_sums", C=C),
               lambda: lib.sd_bn_stats_from_sums(p(sums), C, R.EPS, R.MOMENTUM, p(rm), p(rv), p(mean), p(invstd), st),
               dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv))
        r.call(f"bn_bwd_means_from_sums/C{C}", desc("bn_bwd_means_from_sums", C=C),
               lambda: lib.sd_bn_bwd_means_from_sums(p(sums), C, p(mo), st), dict(means=mo))
        sc, sh = r.out(C), r.out(C)
        gm, bt, m0, v0 = (r.up(t) for t in (q.gamma, q.beta, q.prior0, q.prior1.abs() + 0.5))
        r.call(f"bn_fold/C{C}", desc("bn_fold", C=C), lambda: lib.sd_bn_fold(p(gm), p(bt), p(m0), p(v0), R.EPS, C, p(sc), p(sh), st),
               dict(scale=sc, shift=sh))

    # ---- pooling and the stem tail ------------------------------------------------------------------------------------------------------
    for k, (tag, (B, Hi, Wi, C)) in enumerate(P.FWD_SHAPES.items()):
        d = P.exact_inputs(B, Hi, Wi, C, seed=300 + k)
        Ho, Wo = P.out_size(Hi), P.out_size(Wi)
        par = [r.up(t) for t in (d.mean, d.invstd, d.gamma, d.beta)]
        for form in (0, 1):
            sfx, bf = ("", False) if form == 0 else ("_bf16", True)
            xd = r.up(d.x, bf)
            for pair in (1, 0):
                assert lib.sd_set_option(b"pool_fwd_pair", pair) == 0
                yo, io = r.out((B, Ho, Wo, C), torch.bfloat16 if bf else torch.float32), r.out((B, Ho, Wo, C), torch.uint8)
                fn = getattr(lib, "sd_bn_relu_maxpool_fwd" + sfx)
                r.call(f"bn_relu_maxpool_fwd{sfx}/{tag}/pair{pair}", desc("bn_relu_maxpool_fwd", form, B=B, H=Hi, W=Wi, C=C, pair=pair),
                       lambda: fn(p(xd), B, Hi, Wi, C, *[p(t) for t in par], p(yo), p(io), st), dict(y_pool=yo, idx=io))
            assert lib.sd_set_option(b"pool_fwd_pair", 1) == 0
        xd, yo, io = r.up(d.x), r.out((B, Ho, Wo, C)), r.out((B, Ho, Wo, C), torch.uint8)
        r.call(f"maxpool3x3s2_fwd/{tag}", desc("maxpool_fwd", B=B, H=Hi, W=Wi, C=C),
               lambda: lib.sd_maxpool3x3s2_fwd(p(xd), p(yo), p(io), B, Hi, Wi, C, st), dict(y=yo, idx=io))
        dyd, dxo = r.up(d.dpool), r.out((B, Hi, Wi, C))
        r.call(f"maxpool3x3s2_bwd/{tag}", desc("maxpool_bwd", B=B, H=Hi, W=Wi, C=C),
               lambda: lib.sd_maxpool3x3s2_bwd(p(dyd), p(io), p(dxo), B, Hi, Wi, C, st), dict(dx=dxo))
        x16, y16 = r.up(d.x, True), r.out((B, Ho, Wo, C), torch.bfloat16)
        r.call(f"maxpool3x3s2_fwd_bf16/{tag}", desc("maxpool_fwd", 1, B=B, H=Hi, W=Wi, C=C),
               lambda: lib.sd_maxpool3x3s2_fwd_bf16(p(x16), p(y16), B, Hi, Wi, C, st), dict(y=y16))

    stem_forms = (("", 0, False, torch.float32), ("_bf16", 1, True, torch.float32), ("_bf16_dx16", 2, True, torch.bfloat16))
    for k, (tag, (B, Hi, Wi, C)) in enumerate(list(P.BWD_SHAPES.items()) + list(P.FOLD_SHAPES.items())):
        d = P.exact_inputs(B, Hi, Wi, C, seed=400 + k)
        idx = r.up(P.random_taps(B, Hi, Wi, C, seed=400 + k))
        M = B * Hi * Wi
        nws = lib.sd_col_reduce_workspace_bytes(M, C)
        par = [r.up(t) for t in (d.mean, d.invstd, d.gamma, d.beta)]
        means = r.up(torch.cat([d.mg, d.mgx]))
        acc = k % 2
        for sfx, form, bf, dxt in stem_forms:
            dp, xd = r.up(d.dpool, bf), r.up(d.x, bf)
            dx, dg, db, ws = r.out((B, Hi, Wi, C), dxt), r.out(C, like=d.prior0), r.out(C, like=d.prior1), r.ws(nws)
            fn = getattr(lib, "sd_maxpool_bn_relu_bwd" + sfx)
            r.call(f"maxpool_bn_relu_bwd{sfx}/{tag}/acc{acc}", desc("stem_bwd", form, B=B, H=Hi, W=Wi, C=C),
                   lambda: fn(p(dp), p(idx), p(xd), B, Hi, Wi, C, *[p(t) for t in par], p(dx), p(dg), p(db), acc, p(ws), nws, st),
                   dict(dx=dx, dgamma=dg, dbeta=db, ws=ws), {"col_reduce_workspace_bytes": nws})
            dx = r.out((B, Hi, Wi, C), dxt)
            fn = getattr(lib, "sd_maxpool_bn_relu_bwd_apply" + sfx)
            r.call(f"maxpool_bn_relu_bwd_apply{sfx}/{tag}", desc("stem_bwd_apply", form, B=B, H=Hi, W=Wi, C=C),
                   lambda: fn(p(dp), p(idx), p(xd), B, Hi, Wi, C, *[p(t) for t in par], p(means), p(dx), st), dict(dx=dx))
            if form < 2:
                dg, db, sums, ws = r.out(C, like=d.prior0), r.out(C, like=d.prior1), r.out(2 * C + 1, torch.float64), r.ws(nws)
                fn = getattr(lib, "sd_maxpool_bn_relu_bwd_reduce" + sfx)
                r.call(f"maxpool_bn_relu_bwd_reduce{sfx}/{tag}/acc{acc}", desc("stem_bwd_reduce", form, B=B, H=Hi, W=Wi, C=C, flags=ALL_ALIGNED | F_SUMS),
                       lambda: fn(p(dp), p(idx), p(xd), B, Hi, Wi, C, *[p(t) for t in par], p(dg), p(db), acc, p(sums), p(ws), nws, st),
                       dict(dgamma=dg, dbeta=db, sums=sums, ws=ws))

    for k, (tag, (B, H, W, C)) in enumerate(P.UP_SHAPES.items()):
        g = gen(500 + k)
        dy, add = ints(g, (B, 2 * H, 2 * W, C), 4), ints(g, (B, H, W, C), 4)
        for form, sfx, bf in ((0, "", False), (1, "_bf16", True)):
            dyd = r.up(dy, bf)
            for addd in (None, r.up(add, bf)):
                dx = r.out((B, H, W, C), torch.bfloat16 if bf else torch.float32)
                fn = getattr(lib, "sd_upsample2x_bwd" + sfx)
                r.call(f"upsample2x_bwd{sfx}/{tag}/add{int(addd is not None)}", desc("upsample_bwd", form, B=B, H=H, W=W, C=C),
                       lambda: fn(p(dyd), p(addd), p(dx), B, H, W, C, st), dict(dx=dx))

    for n in (4, 4100, 4098):                                              # the last: n % 4 != 0 is refused
        g = gen(600 + n)
        x = ints(g, (n,), 100)
        xd, y16 = r.up(x), r.out(n, torch.bfloat16)
        r.call(f"cast_f32_to_bf16/n{n}", desc("cast", 0, M=n), lambda: lib.sd_cast_f32_to_bf16(p(xd), p(y16), n, st), dict(y=y16))
        x16, y = r.up(x, True), r.out(n)
        r.call(f"cast_bf16_to_f32/n{n}", desc("cast", 1, M=n), lambda: lib.sd_cast_bf16_to_f32(p(x16), p(y), n, st), dict(y=y))

    # ---- the head ---------------------------------------------------------------------------------------------------------------------------
    head_cases = [c for c in X.EXACT_HEAD_CASES if c[4] <= 32] + [next(c for c in X.EXACT_HEAD_CASES if c[4] > 32)]
    for k, case in enumerate(head_cases):
        B, H, W, C, Co = case
        HW = H * W
        tag = "x".join(map(str, case))
        g = gen(700 + k)
        x, w, b, dy = ints(g, (B, HW, C), 3), ints(g, (Co, C), 2), ints(g, (Co,), 4), ints(g, (B, Co, HW), 3)
        nws = lib.sd_head_bwd_workspace_bytes(B, HW, C, Co)
        sizes = {"head_bwd_workspace_bytes": nws}
        wd, bd, dyd = r.up(w), r.up(b), r.up(dy)
        for off in (False,):                                               # (the head's alignment predicates are covered on the CPU alone)
            al, otag = ALL_ALIGNED, tag
            xd, x16 = r.up(x), r.up(x, True)
            y = r.out((B, Co, HW))
            r.call(f"head_fwd/{otag}", desc("head_fwd", 0, B=B, H=HW, C=C, Co=Co, flags=al),
                   lambda: lib.sd_head_fwd(p(xd), p(wd), p(bd), p(y), B, HW, C, Co, st), dict(y=y), sizes)
            y = r.out((B, Co, HW))
            r.call(f"head_fwd_bf16/{otag}", desc("head_fwd", 1, B=B, H=HW, C=C, Co=Co, flags=al),
                   lambda: lib.sd_head_fwd_bf16(p(x16), p(wd), p(bd), p(y), B, HW, C, Co, st), dict(y=y))
            for acc in (0, 1):
                dx, dw, dbi, ws = r.out((B, HW, C)), r.out((Co, C), like=w), r.out(Co, like=b), r.ws(nws)
                r.call(f"head_bwd/{otag}/acc{acc}", desc("head_bwd", 0, B=B, H=HW, C=C, Co=Co, flags=al),
                       lambda: lib.sd_head_bwd(p(dyd), p(xd), p(wd), p(dx), p(dw), p(dbi), B, HW, C, Co, acc, p(ws), nws, st),
                       dict(dx=dx, dw=dw, dbias=dbi, ws=ws))
    for k, case in enumerate(X.EXACT_HEAD_BF16_BWD_CASES):
        B, H, W, C, Co = case
        HW = H * W
        tag = "x".join(map(str, case))
        g = gen(800 + k)
        x, w, b, dy = ints(g, (B, HW, C), 3), ints(g, (Co, C), 2), ints(g, (Co,), 4), ints(g, (B, Co, HW), 3)
        nws = lib.sd_head_bwd_workspace_bytes(B, HW, C, Co)
        x16, wd, dyd = r.up(x, True), r.up(w), r.up(dy)
        for acc in (0, 1):
            dx, dw, dbi, ws = r.out((B, HW, C), torch.bfloat16), r.out((Co, C), like=w), r.out(Co, like=b), r.ws(nws)
            r.call(f"head_bwd_bf16/{tag}/acc{acc}", desc("head_bwd", 1, B=B, H=HW, C=C, Co=Co),
                   lambda: lib.sd_head_bwd_bf16(p(dyd), p(x16), p(wd), p(dx), p(dw), p(dbi), B, HW, C, Co, acc, p(ws), nws, st),
                   dict(dx=dx, dw=dw, dbias=dbi, ws=ws), {"head_bwd_workspace_bytes": nws})

    # ---- the optimizer ----------------------------------------------------------------------------------------------------------------------
    n = 4100
    g = gen(900)
    prm, grd, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    maskb = (torch.arange(n) % 3 != 0).to(torch.uint8)
    grdd, maskd = r.up(grd), r.up(maskb)
    hyper = (3, 1e-3, 0.9, 0.999, 1e-8, 0.5)                              # step, lr, beta1, beta2, eps, grad_scale
    pd, md, vd = r.up(prm), r.up(m0), r.up(v0)
    r.call("adam_step", desc("adam", M=n), lambda: lib.sd_adam_step(p(pd), p(grdd), p(md), p(vd), n, *hyper, st), dict(param=pd, exp_avg=md, exp_avg_sq=vd))
    nsq = lib.sd_grad_sumsq_workspace_bytes(n)
    partials = r.out(max(nsq // 8, 1), torch.float64)
    r.call("grad_sumsq", desc("grad_sumsq", M=n), lambda: lib.sd_grad_sumsq(p(grdd), n, p(partials), nsq, st), dict(partials=partials),
           {"grad_sumsq_workspace_bytes": nsq})
    for opts in range(8):
        decay, clip, avg = opts & 1, opts >> 1 & 1, opts >> 2 & 1
        pd, md, vd, ema, status = r.up(prm), r.up(m0), r.up(v0), r.up(prm * 0.5), r.up(torch.zeros(4, dtype=torch.int32))
        fl = ALL_ALIGNED | (F_DECAY if decay else 0) | (F_CLIP if clip else 0) | (F_EMA if avg else 0)
        r.call(f"optim_step/decay{decay}_clip{clip}_ema{avg}", desc("optim", M=n, flags=fl),
               lambda: lib.sd_optim_step(p(pd), p(grdd), p(md), p(vd), n, *hyper, 0.01 if decay else 0.0, p(maskd) if decay else None,
                                         1.0 if clip else 0.0, p(partials) if clip else None, nsq // 8 if clip else 0, p(ema) if avg else None,
                                         0.99 if avg else 0.0, p(status) if clip else None, st),
               dict(param=pd, exp_avg=md, exp_avg_sq=vd, ema=ema, status=status))
    return r.calls


# ---- the launch sequences of a run under rocprofv3 --kernel-trace -------------------------------------------------------------------------
def kernel_label(name):
    """`void sd::k_col_reduce<1, float>(float const*, ...)` -> `k_col_reduce<1, float>`: the name as the kernel trace prints it, without the
    return type, the namespace and the parameter list."""
    name = re.sub(r"\.kd$", "", name.strip())
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    name = name[:cut].strip()
    name = re.sub(r"^void\s+", "", name)
    return name.replace("sd::", "").replace("(anonymous namespace)::", "")


def launches_from_csv(path):
    """Per call (one group per separator kernel, in order) the list of `<kernel> grid=X block=N lds=N` of the library's kernels."""
    rows = list(csv.DictReader(open(path, newline="")))
    rows.sort(key=lambda row: (int(row["Start_Timestamp"]), int(row.get("Dispatch_Id", 0) or 0)))
    sep = next(row["Kernel_Name"] for row in rows if "bitwise_not" in row["Kernel_Name"])
    groups = []
    for row in rows:
        if row["Kernel_Name"] == sep:
            groups.append([])
        elif "sd::" in row["Kernel_Name"]:
            wg = int(row["Workgroup_Size_X"]) * int(row.get("Workgroup_Size_Y", 1) or 1) * int(row.get("Workgroup_Size_Z", 1) or 1)
            assert int(row.get("Grid_Size_Y", 1) or 1) == 1 and int(row.get("Grid_Size_Z", 1) or 1) == 1, row
            groups[-1].append(f"{kernel_label(row['Kernel_Name'])} grid={int(row['Grid_Size_X']) // wg} block={wg} lds={int(row.get('LDS_Block_Size') or row.get('Group_Segment_Size') or 0)}")
    return groups[1:]                                                      # (the first separator is the Recorder's own)


class _Table(list):
    """A list that hands out the index of a value, adding it when new."""
    def at(self, value):
        if value not in self:
            self.append(value)
        return self.index(value)


SHAPE_FIELDS = ("B", "H", "W", "M", "C", "Co", "rows")


def build_fixture(run, launches):
    """The fixture: everything that repeats is written once.  Tables `kernels`, `launches` (a launch is `<kernel index> <grid> <lds>`,
    256 threads per block), `digests`, `tags` (case names), `shapes` (SHAPE_FIELDS), `sizes`, `errors`; per entry point its `op`, `form`,
    the names of its output buffers (`out`) and its calls [tag, variant, shape, relu, flags, pool_fwd_pair, launches, sizes or -1,
    digests per output (-1: none) | error], each but `variant` an index into its table.  load_fixture gives the calls back in full."""
    assert len(run) == len(launches) and len({c["name"] for c in run}) == len(run), (len(run), len(launches))
    t = {k: _Table() for k in ("kernels", "launches", "digests", "tags", "shapes", "sizes", "errors")}
    entries = {}
    for rec, seq in zip(run, launches):
        packed = []
        for item in seq:
            label, grid, block, lds = re.fullmatch(r"(.*) grid=(\d+) block=(\d+) lds=(\d+)", item).groups()
            assert block == "256", item
            packed.append(f"{t['kernels'].at(label)} {grid} {lds}")
        assert bool(rec["rc"]) <= (not packed), rec
        entry, _, rest = rec["name"].partition("/")
        tag, _, variant = rest.partition("/")
        d = dict(zip(DESC_FIELDS, rec["desc"]))
        e = entries.setdefault(entry, {"op": d["op"], "form": d["form"], "out": [], "calls": []})
        assert (e["op"], e["form"]) == (d["op"], d["form"]) and rec["rc"] in (0, -1), rec
        e["out"] += [k for k in rec.get("out", {}) if k not in e["out"]]
        result = t["errors"].at(rec["error"]) if rec["rc"] else {k: t["digests"].at(v) for k, v in rec["out"].items()}
        e["calls"].append([t["tags"].at(tag), variant, t["shapes"].at([d[k] for k in SHAPE_FIELDS]), d["relu"], d["flags"], d["pool_fwd_pair"],
                           t["launches"].at(packed), t["sizes"].at(rec["sizes"]) if "sizes" in rec else -1, result])
    for e in entries.values():                          # digests in the order of `out`, -1 for a buffer the call did not have
        for c in e["calls"]:
            if isinstance(c[-1], dict):
                c[-1] = [c[-1].get(k, -1) for k in e["out"]]
    return dict({k: list(v) for k, v in t.items()}, shape_fields=list(SHAPE_FIELDS), entries=entries)


def load_fixture(path=None):
    """{"kernels": [...], "calls": [{"name", "desc", "rc", "error" | "out", "sizes"?, "launches"}]}: the fixture's calls in full."""
    fx = json.loads(Path(path or FIXTURE).read_text())
    calls = []
    for entry, e in fx["entries"].items():
        for tag, variant, shape, relu, flags, pair, seq, sizes, result in e["calls"]:
            d = dict(zip(fx["shape_fields"], fx["shapes"][shape]), op=e["op"], form=e["form"], relu=relu, flags=flags, pool_fwd_pair=pair)
            rec = {"name": "/".join(x for x in (entry, fx["tags"][tag], variant) if x), "desc": [d[k] for k in DESC_FIELDS]}
            if isinstance(result, int):
                rec.update(rc=-1, error=fx["errors"][result])
            else:
                rec.update(rc=0, out={k: fx["digests"][i] for k, i in zip(e["out"], result) if i >= 0})
            if sizes >= 0:
                rec["sizes"] = fx["sizes"][sizes]
            calls.append(dict(rec, launches=fx["launches"][seq]))
    return {"kernels": fx["kernels"], "calls": calls}


def fixture_launches(fx, call):
    out = []
    for item in call["launches"]:
        i, grid, lds = item.split()
        out.append(f"{fx['kernels'][int(i)]} grid={grid} block=256 lds={lds}")
    return out


def dump(obj, path):
    text = json.dumps(obj, separators=(",", ":")).replace('},{"name"', '},\n{"name"').replace('],"', '],\n"').replace('},"', '},\n"')
    if path:
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text(text + "\n")
    else:
        print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("run", "launches", "fixture"))
    ap.add_argument("files", nargs="*"); ap.add_argument("--sep", action="store_true"); ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=None, help="the checkout whose structuredetector_amd is driven (default: this one)")
    a = ap.parse_args()
    if a.root:
        sys.path.insert(0, str(Path(a.root).resolve()))
    if a.mode == "run":
        dump(run_calls(sep=a.sep), a.out)
    elif a.mode == "launches":
        dump(launches_from_csv(a.files[0]), a.out)
    else:
        run, launches = (json.loads(Path(f).read_text()) for f in a.files)
        dump(build_fixture(run, launches), a.out or FIXTURE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
