"""The optimizer options on the GPU: `sd_grad_sumsq` + `sd_optim_step` (AdamW decay, global-norm clipping, weight EMA, the non-finite
guard) against torch on the CPU, and `TrainStep` with the options through resume, `ema_weights()` and model saving.  Expected values
come from torch.optim.AdamW / clip_grad_norm_ and a written-out EMA recurrence in this file, never from the code under test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def f32(x):
    """The value the C ABI receives for a `float` argument, as a Python float."""
    return float(np.float32(x))


# Hyper-parameters cross the C ABI as `float`, so the torch references below are given the fp32-representable values the kernels
# receive.  It matters for beta2: 1 - 0.999 is 1.0e-3 in double but 0.99998713e-3 from the float the kernel is handed; a reference fed
# the double would differ from ANY implementation behind this interface by 1.3e-5 of exp_avg_sq, which says nothing about the kernel.
LR, B1, B2, EPS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
ADAM_TOL = 1e-6          # tests/test_gpu_network.py, `close(pd.cpu(), pr.detach(), 1e-6)`: sd_adam_step against torch.optim.Adam, of the largest value


def sumsq(lib, g, partials=None):
    from structuredetector_amd import _lib as L
    n = g.numel()
    if partials is None:
        partials = torch.empty(lib.sd_grad_sumsq_workspace_bytes(n) // 8, dtype=torch.float64, device=g.device)
    L.check(lib.sd_grad_sumsq(g.data_ptr(), n, partials.data_ptr(), partials.numel() * 8, L.stream()), "sd_grad_sumsq")
    return partials


def optim_step(lib, p, g, m, v, step, gscale=1.0, wd=0.0, mask=None, max_norm=0.0, ema=None, ema_decay=0.0, status=None, partials=None):
    from structuredetector_amd import _lib as L
    if max_norm > 0:
        partials = sumsq(lib, g, partials)
    L.check(lib.sd_optim_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), step, LR, B1, B2, EPS, gscale, wd,
                              None if mask is None else mask.data_ptr(), max_norm, None if partials is None else partials.data_ptr(),
                              0 if partials is None else partials.numel(), None if ema is None else ema.data_ptr(), ema_decay,
                              None if status is None else status.data_ptr(), L.stream()), "sd_optim_step")
    torch.cuda.synchronize()
    return partials


def new_status():
    return torch.zeros(4, dtype=torch.int32, device=DEV)


def read_status(status):
    s = status.cpu()
    return float(s.view(torch.float32)[0]), float(s.view(torch.float32)[1]), int(s[2])


@pytest.mark.parametrize("n", [1000, 4096, 256 * 4 * 7 + 4, (1 << 20) + 12])
def test_all_options_off_is_bit_identical_to_adam_step(n):
    from structuredetector_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    pa, ma, va = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb, mb, vb = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g).to(DEV)
        L.check(lib.sd_adam_step(pa.data_ptr(), gr.data_ptr(), ma.data_ptr(), va.data_ptr(), n, step, LR, B1, B2, EPS, 0.5, L.stream()))
        optim_step(lib, pb, gr, mb, vb, step, gscale=0.5)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa.cpu(), p0)


def _small_step_setup(seed=0, **namespace):
    from structuredetector_amd.data import Encode
    from structuredetector_amd.data.synthetic import synthetic_batch
    from structuredetector_amd.model import Network
    from tests.test_host_cpu import make_args
    dev = torch.device("cuda", 0)
    args = make_args(2, 1, 20, 40, device=dev, learning_rate=1e-3, **namespace)
    torch.manual_seed(seed)
    net = Network(args, pretrained=False).to(dev).train()
    enc = Encode(args)
    batches = []
    for k in range(2):
        tgt = enc.render(enc.plan(128, 128, *synthetic_batch(np.random.default_rng(100 + k), 2, 128, 128, 2, 1)), dev)
        x = torch.randn(2, 3, 128, 128, device=dev, generator=torch.Generator(dev).manual_seed(200 + k))
        batches.append((x, tgt))
    return args, net, batches


class _Spy:
    """Stands in for the library handle: records the name of every entry point that is looked up on it."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


def test_default_train_step_calls_adam_step_and_options_call_optim_step(monkeypatch):
    from structuredetector_amd import _lib as L
    from structuredetector_amd.model.trainer import TrainStep
    args, net, batches = _small_step_setup()
    real = L.lib()
    for kw, want, never in (({}, {"sd_adam_step"}, {"sd_optim_step", "sd_grad_sumsq"}),
                            (dict(weight_decay=0.01), {"sd_optim_step"}, {"sd_adam_step", "sd_grad_sumsq"}),
                            (dict(ema_decay=0.9), {"sd_optim_step"}, {"sd_adam_step", "sd_grad_sumsq"}),
                            (dict(clip_grad_norm=1.0), {"sd_optim_step", "sd_grad_sumsq"}, {"sd_adam_step"})):
        step = TrainStep(net, args, **kw)
        assert step.plain_adam == (not kw)
        spy = _Spy(real)
        monkeypatch.setattr(L, "_lib", spy)
        step(*batches[0])
        torch.cuda.synchronize()
        monkeypatch.setattr(L, "_lib", real)
        called = set(spy.calls)
        assert want <= called and not (never & called), (kw, sorted(called))


def _torch_reference(dtype, p0, grads, elem_mask, wd, max_norm, ema_decays):
    """torch.optim.AdamW over two parameter groups (decayed / not decayed), clip_grad_norm_ before each step, the EMA recurrence written
    out.  Returns the flat parameters, moments, EMA and the per-step norms."""
    dec = p0[elem_mask].to(dtype).clone().requires_grad_(True)
    rest = p0[~elem_mask].to(dtype).clone().requires_grad_(True)
    opt = torch.optim.AdamW([dict(params=[dec], weight_decay=wd), dict(params=[rest], weight_decay=0.0)], lr=LR, betas=(B1, B2), eps=EPS)
    ema = p0.to(dtype).clone()
    norms = []

    def flat(a, b):
        out = torch.empty(p0.numel(), dtype=dtype)
        out[elem_mask], out[~elem_mask] = a, b
        return out

    for gr, d in zip(grads, ema_decays):
        gr = gr.to(dtype)
        dec.grad, rest.grad = gr[elem_mask].clone(), gr[~elem_mask].clone()
        if max_norm > 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_([dec, rest], max_norm)))
        else:
            norms.append(float(gr.double().norm()))
        opt.step()
        ema = d * ema + (1 - d) * flat(dec.detach(), rest.detach())
    m = flat(opt.state[dec]["exp_avg"], opt.state[rest]["exp_avg"])
    v = flat(opt.state[dec]["exp_avg_sq"], opt.state[rest]["exp_avg_sq"])
    return flat(dec.detach(), rest.detach()), m, v, ema, norms


N_TAIL = 256 * 4 * 48 + 20           # 48 full blocks and a tail of five float4


@pytest.mark.parametrize("case", ["off", "below", "far_above", "within_an_ulp"])
def test_five_steps_against_torch_adamw_clip_and_ema(case):
    """Truth: the torch reference in fp64; yardstick: the same in fp32 (printed beside each figure, `pytest -s`).  Bound on the largest
    error against the truth, for every case and every buffer (parameters, both moments, EMA): the Adam tolerance of
    tests/test_gpu_network.py, 1e-6 of the largest value.  The looser bound the issue allows where clipping needs it (twice the error
    of torch's own fp32 run) is not used.  The norm of the status block: 1e-6 relative to the fp64 norm."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n, wd, gscale = N_TAIL, f32(0.05), 0.5
    g = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g)
    mask = (torch.rand(n // 4, generator=g) < 0.6).to(torch.uint8)
    elem_mask = mask.repeat_interleave(4).bool()
    grads = [torch.randn(n, generator=g) * 0.02 for _ in range(5)]          # the averaged gradients; the kernel is fed 2 x with grad_scale 0.5
    typical = float(grads[0].double().norm())
    if case == "within_an_ulp":              # every gradient rescaled to a norm of 1 up to fp32 rounding, clipped at exactly 1
        grads = [(gr.double() / gr.double().norm()).float() for gr in grads]
        max_norm = 1.0
        for gr in grads:
            assert abs(float(gr.double().norm()) - 1.0) < 2 ** -23
    else:
        max_norm = f32({"off": 0.0, "below": 10 * typical, "far_above": 0.01 * typical}[case])
    ema_decays = [f32(min(0.99, (1 + t) / (10 + t))) for t in range(1, 6)]
    want = _torch_reference(torch.float64, p0, grads, elem_mask, wd, max_norm, ema_decays)
    yard = _torch_reference(torch.float32, p0, grads, elem_mask, wd, max_norm, ema_decays)

    def run(max_norm):
        p, m, v, ema = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), p0.to(DEV)
        status, seen = new_status(), []
        for step, (gr, d) in enumerate(zip(grads, ema_decays), 1):
            optim_step(lib, p, (gr * 2).to(DEV), m, v, step, gscale=gscale, wd=wd, mask=mask.to(DEV), max_norm=max_norm, ema=ema, ema_decay=d,
                       status=status)
            seen.append(read_status(status))
        return (p.cpu(), m.cpu(), v.cpu(), ema.cpu()), seen

    got, seen = run(max_norm)
    for name, a, w, y in zip(("param", "exp_avg", "exp_avg_sq", "ema"), got, want, yard):
        scale = w.abs().max().item()
        err, err32 = (a.double() - w).abs().max().item(), (y.double() - w).abs().max().item()
        print(f"{case} {name}: err/scale {err / scale:.3e}, torch fp32 err/scale {err32 / scale:.3e}")
        assert err <= ADAM_TOL * scale, f"{case} {name}: {err:.3e} vs fp64, torch fp32 {err32:.3e}, scale {scale:.3e}"
    if case != "off":
        for (norm, coef, skipped), norm64 in zip(seen, want[4]):
            print(f"{case} norm: {norm!r} vs {norm64!r} rel {abs(norm - norm64) / norm64:.3e} coef {coef!r}")
            assert abs(norm - norm64) <= 1e-6 * norm64 and skipped == 0
            if case == "below":
                assert coef == 1.0
            elif case == "far_above":
                assert coef == pytest.approx(max_norm / norm64, rel=1e-5)
            else:
                assert 1.0 - 4e-6 <= coef <= 1.0
    if case == "below":                      # a coefficient of exactly 1: the bits of a run without clipping
        unclipped, _ = run(0.0)
        for a, b in zip(got, unclipped):
            assert torch.equal(a, b)


def test_reduction_and_step_are_deterministic_and_ignore_the_workspace_contents():
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n = 5_000_004                                 # more float4 than 512 blocks x 256 threads x 8 loads cover in one sweep, plus a ragged end
    g = torch.Generator().manual_seed(11)
    gr = (torch.randn(n, generator=g) * 3).to(DEV)
    p0 = torch.randn(n, generator=g)
    count = lib.sd_grad_sumsq_workspace_bytes(n) // 8
    assert count == 512
    runs = []
    for fill in (0.0, float("nan"), 1e300):
        partials = torch.full((count,), fill, dtype=torch.float64, device=DEV)
        p, m, v, status = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), new_status()
        optim_step(lib, p, gr, m, v, 1, max_norm=1.0, status=status, partials=partials)
        runs.append((partials.cpu(), status.cpu(), p.cpu(), m.cpu(), v.cpu()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    total, want = float(runs[0][0].sum()), float((gr.double().cpu() ** 2).sum())
    assert abs(total - want) <= 1e-12 * want
    norm, coef, skipped = read_status(runs[0][1].to(DEV))
    assert abs(norm - want ** 0.5) <= 1e-6 * want ** 0.5 and 0 < coef < 1e-3 and skipped == 0


def test_decay_mask_on_a_real_network_and_a_decay_only_step():
    from structuredetector_amd.model.trainer import TrainStep
    finals = {}
    for wd in (0.0, 0.1):
        args, net, batches = _small_step_setup(seed=5)
        step = TrainStep(net, args, weight_decay=wd)
        step(*batches[0])
        torch.cuda.synchronize()
        finals[wd] = net.flat_params.clone()
    mask = step.decay_mask
    assert mask.dtype == torch.uint8 and mask.numel() * 4 == net.flat_params.numel()
    per_float = mask.repeat_interleave(4).bool()
    covered = torch.zeros_like(per_float)
    convs = others = 0
    for p in net._flat_order:
        off, n = net._flat_off[id(p)]
        a, b = finals[0.0][off:off + n], finals[0.1][off:off + n]
        if p.dim() == 4:
            convs += 1
            assert bool(per_float[off:off + n].all())
            covered[off:off + n] = True
            assert not torch.equal(a, b) and float((a != b).float().mean()) > 0.9, "a decayed step must change the conv weight"
        else:
            others += 1
            assert not bool(per_float[off:off + n].any())
            assert torch.equal(a, b), "biases and BatchNorm parameters must not be decayed"
    assert convs > 30 and others > 60
    assert torch.equal(covered, per_float), "flags outside the 4-D tensors"


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_skips_the_step_and_the_next_clean_step_is_unaffected(bad):
    """An arithmetic check on values in a buffer: one inf (nan) among the gradient values makes the norm non-finite; the launch then
    stores nothing but the status block."""
    from structuredetector_amd import _lib as L
    lib = L.lib()
    n = 256 * 4 * 9 + 8
    g = torch.Generator().manual_seed(3)
    p0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
    e0 = torch.randn(n, generator=g)
    mask = (torch.rand(n // 4, generator=g) < 0.5).to(torch.uint8).to(DEV)
    clean = (torch.randn(n, generator=g) * 0.1).to(DEV)
    poisoned = clean.clone()
    poisoned[n // 3] = bad
    kw = dict(wd=0.05, mask=mask, max_norm=1.0, ema_decay=0.9)
    # with the bad batch: step 4 is skipped, step 5 is clean
    p, m, v, ema, status = p0.to(DEV), m0.to(DEV), v0.to(DEV), e0.to(DEV), new_status()
    optim_step(lib, p, poisoned, m, v, 4, ema=ema, status=status, **kw)
    norm, coef, skipped = read_status(status)
    assert not np.isfinite(norm) and coef == 0.0 and skipped == 1
    for held, first in ((p, p0), (m, m0), (v, v0), (ema, e0)):
        assert torch.equal(held.cpu(), first)
    optim_step(lib, p, poisoned, m, v, 4, ema=ema, status=status, **kw)
    assert read_status(status)[2] == 2 and torch.equal(p.cpu(), p0)
    optim_step(lib, p, clean, m, v, 5, ema=ema, status=status, **kw)
    norm, coef, skipped = read_status(status)
    assert np.isfinite(norm) and 0 < coef < 1 and skipped == 2
    # without the bad batch: the same clean step, same `step` argument
    q, mq, vq, eq, status_q = p0.to(DEV), m0.to(DEV), v0.to(DEV), e0.to(DEV), new_status()
    optim_step(lib, q, clean, mq, vq, 5, ema=eq, status=status_q, **kw)
    assert read_status(status_q)[2] == 0
    assert torch.equal(p, q) and torch.equal(m, mq) and torch.equal(v, vq) and torch.equal(ema, eq)
    assert not torch.equal(q.cpu(), p0)


OPTIONS = dict(weight_decay=0.05, clip_grad_norm=0.5, ema_decay=0.9)


@pytest.mark.parametrize("amp", [False, True])
def test_train_step_resume_ema_weights_and_saved_best_model(amp, tmp_path):
    from structuredetector_amd.model import Network
    from structuredetector_amd.model.trainer import TrainStep
    # four steps in one go
    args, net, batches = _small_step_setup(seed=9, use_amp=amp)
    step = TrainStep(net, args, **OPTIONS)
    assert step.amp == amp
    for k in range(4):
        step(*batches[k % 2])
    torch.cuda.synchronize()
    assert float(step.grad_norm) > 0 and int(step.skipped_steps) == 0 and 0 < float(step.clip_coef) <= 1
    # two steps, a checkpoint through a file, a fresh network and a fresh step without the options, two more steps
    args2, net2, _ = _small_step_setup(seed=9, use_amp=amp)
    step2 = TrainStep(net2, args2, **OPTIONS)
    for k in range(2):
        step2(*batches[k % 2])
    torch.save({"model": {k: v.detach().cpu().clone() for k, v in net2.state_dict().items()}, "optimizer": step2.state_dict()}, tmp_path / "resume.pth")
    state = torch.load(tmp_path / "resume.pth", map_location="cpu", weights_only=True)
    assert state["optimizer"]["ema_decay"] == 0.9 and state["optimizer"]["skipped_steps"] == 0
    net3 = Network(args2, pretrained=False).to(args2.device).train()
    net3.load_state_dict(state["model"])
    step3 = TrainStep(net3, args2)
    assert step3.plain_adam and step3.ema is None
    step3.load_state_dict(state["optimizer"])
    assert not step3.plain_adam and (step3.weight_decay, step3.clip_grad_norm, step3.ema_decay) == (0.05, 0.5, 0.9)
    assert torch.equal(step3.ema, step2.ema)
    for k in range(2, 4):
        step3(*batches[k % 2])
    torch.cuda.synchronize()
    assert torch.equal(net3.flat_params, net.flat_params), "resumed run diverged from the uninterrupted one"
    assert torch.equal(step3.ema, step.ema) and torch.equal(step3.exp_avg, step.exp_avg) and torch.equal(step3.exp_avg_sq, step.exp_avg_sq)
    assert not torch.equal(step.ema, net.flat_params)
    # ema_weights(): the averaged weights are in place inside, the raw ones are back afterwards, bit for bit
    raw, avg = net.flat_params.clone(), step.ema.clone()
    x = batches[0][0]
    with step.ema_weights():
        assert torch.equal(net.flat_params, avg) and torch.equal(step.ema, raw)
        net.eval()
        with torch.no_grad():
            inside = net(x)["anchor_hm"]._base.clone()
        net.save(tmp_path / "model_best_loss.pth")
        net.train()
    assert torch.equal(net.flat_params, raw) and torch.equal(step.ema, avg)
    best = Network(args, pretrained=False).to(args.device)
    best.load_state_dict(torch.load(tmp_path / "model_best_loss.pth", map_location="cpu", weights_only=True))
    best.eval()
    net.eval()
    with torch.no_grad():
        assert torch.equal(best(x)["anchor_hm"]._base, inside), "model_best must hold the averaged weights"
        assert not torch.equal(net(x)["anchor_hm"]._base, inside)
    net.train()


def test_resume_state_written_without_the_options_loads_with_them_off():
    from structuredetector_amd.model.trainer import TrainStep
    args, net, batches = _small_step_setup(seed=2)
    plain = TrainStep(net, args)
    plain(*batches[0])
    old = plain.state_dict()
    assert set(old) == {"exp_avg", "exp_avg_sq", "step_count", "lr", "betas", "eps", "flat_numel"}     # the keys of a file written before the options existed
    step = TrainStep(net, args, **OPTIONS)
    step.load_state_dict(old)
    assert step.plain_adam and step.ema is None and step.step_count == 1 and int(step.skipped_steps) == 0


def test_trainer_validates_and_saves_best_models_on_the_averaged_weights(tmp_path, monkeypatch, capsys):
    """`Trainer` with the three options on, one epoch of two steps on synthetic scenes: the validation pass and its `model_best_*.pth`
    files run on the EMA, `last_model.pth` holds the raw weights, `resume.pth` both, the scalars carry the norm of every step and the
    skip count; resuming that run without the flags keeps the checkpoint's options and says so."""
    import json

    from structuredetector_amd.model.trainer import Trainer
    from structuredetector_amd.utils.args import Arguments
    (tmp_path / "labels.json").write_text(json.dumps({"labels": ["bean", "maize"], "parts": ["leaf"]}))
    monkeypatch.chdir(tmp_path)
    argv = ["-W", "128", "-H", "128", "-s", "stem", "--labels", str(tmp_path / "labels.json"), "--synthetic", "8", "-b", "4", "-e", "1"]
    options = ["--weight_decay", "0.05", "--clip_grad_norm", "0.5", "--ema_decay", "0.9"]
    tr = Trainer(Arguments().parse(argv + options))
    seen = []
    inner = tr._valid
    monkeypatch.setattr(tr, "_valid", lambda: (seen.append(tr.net.flat_params.clone()), inner())[1])
    tr.train()
    assert tr.step.step_count == 2 and not tr.step.plain_adam
    raw, avg = tr.net.flat_params.clone(), tr.step.ema.clone()
    assert not torch.equal(raw, avg)
    assert len(seen) == 1 and torch.equal(seen[0], avg), "the validation pass must see the averaged weights"
    with tr.step.ema_weights():
        want_best = {k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()}
    want_last = {k: v.detach().cpu().clone() for k, v in tr.net.state_dict().items()}
    assert torch.equal(tr.net.flat_params, raw)
    best = torch.load(tr.save_dir / "model_best_loss.pth", map_location="cpu", weights_only=True)
    last = torch.load(tr.save_dir / "last_model.pth", map_location="cpu", weights_only=True)
    assert set(best) == set(last) == set(want_best)
    differ = 0
    for k in want_best:
        assert torch.equal(best[k], want_best[k]), f"model_best_loss.pth: {k} is not the averaged weight"
        assert torch.equal(last[k], want_last[k]), f"last_model.pth: {k} is not the raw weight"
        differ += int(not torch.equal(best[k], last[k]))
    assert differ > 100
    state = torch.load(tr.save_dir / "resume.pth", map_location="cpu", weights_only=True)
    assert torch.equal(state["optimizer"]["ema"], avg.cpu())
    assert all(torch.equal(state["model"][k], want_last[k]) for k in want_last), "resume.pth carries the raw weights beside the EMA"
    rows = [json.loads(ln) for ln in (tr.save_dir / "scalars.jsonl").read_text().splitlines()]
    norms = [r for r in rows if r["tag"] == "Gradient norm"]
    assert len(norms) == 2 and all(r["value"] > 0 and np.isfinite(r["value"]) for r in norms)
    assert norms[-1]["value"] == float(tr.step.grad_norm)
    assert [r["value"] for r in rows if r["tag"] == "Skipped steps"] == [0.0]
    capsys.readouterr()
    tr2 = Trainer(Arguments().parse(argv + ["--resume", str(tr.save_dir / "resume.pth")]))
    assert (tr2.step.weight_decay, tr2.step.clip_grad_norm, tr2.step.ema_decay) == (0.05, 0.5, 0.9) and torch.equal(tr2.step.ema, avg)
    assert "optimizer options come from the checkpoint" in capsys.readouterr().out
