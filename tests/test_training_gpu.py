"""The reference's training step on the HIP path: noisy latents, model prediction and loss
against the imported reference's values (tests/golden/tiny_train.npz), and the backward half — two optimisation steps
(backward, clip_grad_norm_ 1.0, AdamW) against what the reference's own modules produce under torch autograd +
torch.optim.AdamW (tests/golden/tiny_train_backward.npz: loss, gradient norm, step-1 gradients of named tensors and
their movement after two steps), plus the backward kernels one by one against torch autograd on the CPU."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mirrorfusion_ref as R  # noqa: E402
from reflecting_reality_amd import DDPMScheduler, hip, models as M, synth  # noqa: E402
from reflecting_reality_amd import ops  # noqa: E402
from reflecting_reality_amd.training import (AdamW, MirrorFusionModel, clip_grad_norm_, compute_snr, load_state, save_state,  # noqa: E402
                                             train_step, training_loss)
from util import golden, keys, report  # noqa: E402

DEV = "cuda"
SD_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _inputs():
    g = torch.Generator().manual_seed(2024)
    return (torch.randn(3, 4, 8, 8, generator=g) * 0.8, torch.randn(3, 4, 8, 8, generator=g),
            torch.randn(3, 5, 8, 8, generator=g), torch.randn(3, 77, 32, generator=g))


def _model(prec):
    unet = M.UNet2DConditionModel(dict(R.TINY_UNET), precision=prec, device=DEV)
    unet.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    bn = M.BrushNetModel(dict(R.brushnet_config(R.TINY_UNET, 5)), precision=prec, device=DEV)
    bn.load_state_dict(synth.state_dict_for(keys("tiny_train")["brushnet"], 21))
    return MirrorFusionModel(unet, bn)


@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_training_loss_matches_reference(prec, ptype):
    G = golden("tiny_train.npz")
    latents, noise, cond, ehs = (t.to(DEV) for t in _inputs())
    ts = torch.from_numpy(G["timesteps"])
    ns = DDPMScheduler(prediction_type=ptype, **SD_SCHED)
    noisy = ns.add_noise(latents, noise, ts)
    report(f"noisy latents {ptype}", noisy, G[f"{ptype}_noisy"], atol=1e-6, rtol=1e-6)
    model = _model(prec)
    tol = dict(atol=2e-4, rtol=2e-4) if prec == "fp32" else dict(atol=6e-2, rtol=6e-2)
    for gamma, tag in ((None, "none"), (5.0, "snr5")):
        loss, pred, target = training_loss(model, ns, latents, noise, ts, ehs, cond, snr_gamma=gamma)
        report(f"model_pred {ptype} [{prec}]", pred, G[f"{ptype}_pred"], **tol)
        ref = float(G[f"{ptype}_loss_{tag}"])
        rel = abs(float(loss.item()) - ref) / ref
        print(f"loss {ptype} gamma={gamma} [{prec}]: {float(loss.item()):.7f} vs reference {ref:.7f} (rel {rel:.2e})")
        assert rel < (1e-4 if prec == "fp32" else 2e-2)


def test_mse_loss_kernel_against_torch():
    """mf_mse_loss on ragged sizes: per-sample means x weights, then the batch mean (F.mse_loss semantics)."""
    g = torch.Generator().manual_seed(3)
    for rows, n in ((1, 1), (3, 257), (5, 4 * 64 * 64), (64, 1000)):
        p = torch.randn(rows, n, generator=g)
        t = torch.randn(rows, n, generator=g)
        w = torch.rand(rows, generator=g) + 0.1
        loss, per = hip.mse_loss(p.to(DEV), t.to(DEV), w.to(DEV))
        ref_per = ((p.double() - t.double()) ** 2).mean(1) * w.double()
        assert torch.allclose(per.cpu().double(), ref_per, rtol=1e-6, atol=1e-7)
        assert abs(float(loss.item()) - float(ref_per.mean())) < 1e-6 * max(1.0, float(ref_per.mean()))
        loss2, _ = hip.mse_loss(p.to(DEV), t.to(DEV))
        ref = torch.nn.functional.mse_loss(p, t)
        assert abs(float(loss2.item()) - float(ref)) < 1e-6 * max(1.0, float(ref))
    with pytest.raises(ValueError):
        hip.mse_loss(torch.zeros(2, 4, device=DEV), torch.zeros(2, 5, device=DEV))


def test_compute_snr_and_velocity_match_oracle_tables():
    ns = DDPMScheduler(**SD_SCHED)
    ts = torch.tensor([0, 17, 480, 999])
    ac = R._alphas_cumprod(R.SD15_SCHED)
    snr = compute_snr(ns, ts)
    assert torch.equal(snr, ((ac ** 0.5)[ts].float() / ((1 - ac) ** 0.5)[ts].float()) ** 2)
    x = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    e = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    v = ns.get_velocity(x.to(DEV), e.to(DEV), ts)
    sa, sb = (ac[ts] ** 0.5)[:, None, None, None], ((1 - ac[ts]) ** 0.5)[:, None, None, None]
    report("velocity", v, sa * e - sb * x, atol=1e-6, rtol=1e-6)


BATCH2 = None


def _batches():
    g2 = torch.Generator().manual_seed(2025)
    lat, noi, cond, ehs = _inputs()
    b2 = (torch.randn(3, 4, 8, 8, generator=g2) * 0.8, torch.randn(3, 4, 8, 8, generator=g2), torch.tensor([702, 3, 250]).long(),
          torch.randn(3, 77, 32, generator=g2), torch.randn(3, 5, 8, 8, generator=g2))
    return [(lat, noi, torch.tensor([17, 480, 965]).long(), ehs, cond), b2]


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("tag,train_unet,gamma", [("frozen", False, None), ("unet", True, 5.0)])
def test_two_training_steps_match_reference(prec, tag, train_unet, gamma):
    """SURVEY.md §8 a-16's pin: (loss, grad-norm, step-1 gradients, |dw| after two AdamW steps) of the HIP training step
    against the reference's modules under torch autograd (fixture generated by tools/make_golden.py::tiny_train)."""
    G = golden("tiny_train_backward.npz")
    model = _model(prec).prepare_training(train_base_unet=train_unet)
    assert [m is model.brushnet for m in model.get_trainable_modules()] == ([False, True] if train_unet else [True])
    w0 = {("unet." if m is model.unet else "") + k: v.clone() for m in model.get_trainable_modules() for k, v in m.state_dict().items()}
    ns = DDPMScheduler(**SD_SCHED)
    opt = AdamW(model.get_trainable_modules(), lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    for i, (lat, noi, ts, ehs, cond) in enumerate(_batches()):
        loss, norm = train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV), snr_gamma=gamma,
                                max_grad_norm=1.0)
        ref_l, ref_n = float(G[f"{tag}_loss_{i}"]), float(G[f"{tag}_grad_norm_{i}"])
        print(f"[{tag} {prec}] step {i}: loss {float(loss):.7f} (ref {ref_l:.7f})  grad norm {float(norm):.6f} (ref {ref_n:.6f})")
        assert abs(float(loss) - ref_l) < 1e-4 * ref_l
        if i == 0:
            grads = {("unet." if m is model.unet else "") + k: v / model.loss_scale for m in model.get_trainable_modules()
                     for k, v in m.grad_state_dict().items()}
            bad = []
            for key in [k for k in G.files if k.startswith(f"{tag}_grad/")]:
                name = key.split("/", 1)[1]
                ref = torch.from_numpy(G[key])
                err = float((grads[name] - ref).abs().max())
                scale = float(ref.abs().max())
                print(f"   grad {name}: max err {err:.3e} (|ref| max {scale:.3e})")
                assert tuple(grads[name].shape) == tuple(ref.shape)
                bad.append(name) if err > 2e-4 * scale + 1e-7 else None
            assert not bad, bad
        assert abs(float(norm) - ref_n) < 2e-4 * ref_n
    w2 = {("unet." if m is model.unet else "") + k: v for m in model.get_trainable_modules() for k, v in m.state_dict().items()}
    for key in [k for k in G.files if k.startswith(f"{tag}_dw/")]:
        name = key.split("/", 1)[1]
        dw = float((w2[name] - w0[name]).norm())
        print(f"   |dw| {name}: {dw:.6e} (ref {float(G[key]):.6e})")
        assert abs(dw - float(G[key])) < 2e-3 * float(G[key]), name
    if not train_unet:         # a frozen UNet keeps its weights and has no gradient arena
        assert model.unet.flat_g is None


def test_bf16x1_training_step_inside_the_reference_mixed_precision_envelope():
    """precision='bf16x1' (fp32 storage, operands rounded to bf16 for one MFMA per product: the arithmetic of
    --mixed_precision=bf16): the first training step's loss, gradient norm and named gradients against the reference's
    fp32 step, held to the deviation the REFERENCE ITSELF shows under bf16 mixed precision on the same case
    (tests/golden/bf16_train_envelope.json, tools/make_bf16_train_envelope.py: rel-L2 0.017-0.030 per tensor).  fp32
    storage rounds less than autocast does, so the bound is 1.0 x the reference's own deviation per tensor."""
    import json
    G = golden("tiny_train_backward.npz")
    with open(os.path.join(os.path.dirname(__file__), "golden", "bf16_train_envelope.json")) as f:
        env = json.load(f)
    model = _model("bf16x1").prepare_training(train_base_unet=False)
    ns = DDPMScheduler(**SD_SCHED)
    opt = AdamW(model.get_trainable_modules(), lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    lat, noi, ts, ehs, cond = _batches()[0]
    loss, norm = train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV), max_grad_norm=1.0)
    # a power-of-two loss scale (exact; bf16 rounding is invariant under it) keeps dO out of the fp16 subnormals of the split
    # flash attention this mode shares with f16x3 at >= 256 tokens (round 4, found by the full-size reference gradients)
    assert model.loss_scale == float(2 ** int(3 * 4 * 8 * 8 - 1).bit_length())
    ref_l, ref_n = float(G["frozen_loss_0"]), float(G["frozen_grad_norm_0"])
    print(f"[bf16x1] loss {float(loss):.7f} (fp32 ref {ref_l:.7f}, reference-bf16 dev {env['loss']['abs_dev']:.2e})  "
          f"grad norm {float(norm):.6f} (ref {ref_n:.6f}, reference-bf16 rel dev {env['grad_norm']['rel_dev']:.2e})")
    # one scalar: the reference's own bf16 deviation of it (4.9e-5) is a lucky cancellation, not a scale; 2^-9 products
    # give a few 1e-4 relative
    assert abs(float(loss) - ref_l) <= 2e-3 * ref_l
    assert abs(float(norm) - ref_n) / ref_n <= max(2.0 * env["grad_norm"]["rel_dev"], 2e-3)
    grads = model.brushnet.grad_state_dict()
    worst = 0.0
    for name, e in env["grads"].items():
        ref = torch.from_numpy(G[f"frozen_grad/{name}"]).float()
        got = grads[name].float().cpu() / model.loss_scale
        rel = float((got - ref).norm() / ref.norm())
        worst = max(worst, rel / e["rel_l2"])
        print(f"   grad {name}: rel-L2 {rel:.4f} (reference under bf16: {e['rel_l2']:.4f})")
        assert rel <= 1.0 * e["rel_l2"], name
    print(f"   worst ratio to the reference's own bf16 deviation: {worst:.2f}")


@pytest.mark.parametrize("prec_name", ["fp32", "bf16x1"])
def test_step_without_the_arena_memset_equals_the_cleared_arena(prec_name):
    """train_step clears only the small accumulated parameters and lets each conv / linear weight's first weight gradient of the
    step WRITE (models.zero_grad_for_step): with the gradient arena poisoned with NaN beforehand, the step's gradients, norm and
    updated weights are bit-identical to the step that memsets the whole arena; with gradient accumulation the second micro-step
    adds; a weight no backward pass reaches is cleared."""
    from reflecting_reality_amd import training as T
    ns = DDPMScheduler(**SD_SCHED)
    lat, noi, ts, ehs, cond = _batches()[0]

    def run(first_write, accum):
        T.FIRST_WRITE = first_write
        try:
            model = _model(prec_name).prepare_training()
            opt = AdamW(model.get_trainable_modules())
            if first_write:
                for m in model.get_trainable_modules():          # (the parameters only: the alignment slack between them stays 0)
                    for prm, _ in m._plist:
                        if prm.grad is not None:
                            prm.grad.fill_(float("nan"))
            for _ in range(accum):
                loss, norm = train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV), gradient_accumulation_steps=accum)
            return float(loss), float(norm), [m.flat_g.clone() for m in model.get_trainable_modules()], [m.flat_w.clone() for m in model.get_trainable_modules()], model
        finally:
            T.FIRST_WRITE = True

    for accum in (1, 2):
        a, b = run(True, accum), run(False, accum)
        assert a[0] == b[0] and a[1] == b[1] and np.isfinite(a[1])
        for ga, gb in zip(a[2], b[2]):
            assert torch.equal(ga, gb)
        for wa, wb in zip(a[3], b[3]):
            assert torch.equal(wa, wb)
    # a weight nothing reaches: marked fresh by zero_grad_for_step, cleared by finish_fresh
    model = a[4]
    bn = model.brushnet
    bn.flat_g.fill_(7.0)
    bn.zero_grad_for_step()
    assert all(p.fresh for p in bn._fw_params) and float(bn._fw_params[0].grad.abs().max()) == 7.0
    small = [p for p, _ in bn._plist if p.grad is not None and all(p is not q for q in bn._fw_params)]
    assert small and all(float(p.grad.abs().max()) == 0.0 for p in small)
    bn.finish_fresh()
    assert not any(p.fresh for p in bn._fw_params) and float(bn.flat_g[: bn.num_arena_floats()].abs().max()) == 0.0


def test_training_step_is_deterministic_and_checkpoints_resume(tmp_path):
    """Two identical runs give bit-identical weights (fixed-order reductions, no atomics); save_state writes
    checkpoint-N/{brushnet} in the reference's layout, rotates old checkpoints, and load_state resumes: step 2 after a
    reload equals step 2 of the uninterrupted run."""
    ns = DDPMScheduler(**SD_SCHED)
    batches = _batches()

    def run(stop_and_resume):
        model = _model("fp32").prepare_training()
        opt = AdamW(model.get_trainable_modules())
        lat, noi, ts, ehs, cond = batches[0]
        train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV))
        if stop_and_resume:
            out = str(tmp_path / "run")
            for step in (1, 2, 3):
                path = save_state(out, step, model, opt, checkpoints_total_limit=2)
            import os
            assert sorted(os.listdir(out)) == ["checkpoint-2", "checkpoint-3"]
            assert sorted(os.listdir(path)) == ["brushnet", "optimizer.bin", "trainer_state.json"]
            assert sorted(os.listdir(os.path.join(path, "brushnet"))) == ["config.json", "diffusion_pytorch_model.safetensors"]
            model = _model("fp32").prepare_training()
            opt = AdamW(model.get_trainable_modules())
            assert load_state(path, model, opt) == 3 and opt.step_count == 1
        lat, noi, ts, ehs, cond = batches[1]
        train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV))
        return model.brushnet.state_dict()

    a, b, c = run(False), run(False), run(True)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two identical runs differ"
        assert torch.equal(a[k], c[k]), f"{k}: resuming from the checkpoint changes step 2"
    # the checkpoint's weights load into an inference model of the same class (reference layout on disk)
    import os
    bn = M.BrushNetModel.from_pretrained(os.path.join(str(tmp_path / "run"), "checkpoint-3"), subfolder="brushnet",
                                         precision="fp32", device=DEV)
    assert set(bn.state_dict()) == set(a)


@pytest.mark.parametrize("prec,snr_gamma", [("f16x3", None), ("fp32", 5.0), ("bf16x1", None)])
def test_graphed_train_step_equals_the_eager_one(prec, snr_gamma):
    """GraphedTrainStep (zero_grad + forward + loss + backward + clip replayed from one hipGraph; noising, SNR weights, range
    guard and AdamW eager around it) leaves bit-identical weights, loss and gradient norm to train_step over five steps with
    changing inputs and timesteps (two eager warm-up calls, the capture, two replays)."""
    from reflecting_reality_amd.training import GraphedTrainStep
    ns = DDPMScheduler(**SD_SCHED)
    batches = _batches()

    def run(graphed):
        model = _model(prec).prepare_training()
        opt = AdamW(model.get_trainable_modules())
        step = GraphedTrainStep(model, ns, opt, snr_gamma=snr_gamma, warmup=2) if graphed else None
        out = []
        for i in range(5):
            lat, noi, ts, ehs, cond = batches[i % len(batches)]
            ts = (ts + 37 * i) % 1000
            args = (lat.to(DEV) * (1.0 + 0.1 * i), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV))
            loss, norm = step(*args) if graphed else train_step(model, ns, opt, *args, snr_gamma=snr_gamma)
            out.append((float(loss), float(norm)))
        if graphed:
            assert step.graph is not None and step.calls == 5
        return model.brushnet.state_dict(), out

    (wa, la), (wb, lb) = run(False), run(True)
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), f"{k}: the graphed step differs from the eager one"


def test_training_needs_fp32_class_precision_and_the_training_layout():
    model = _model("bf16")
    with pytest.raises(NotImplementedError, match="fp32 master"):
        model.brushnet.train()
    m32 = _model("fp32")
    lat, noi, cond, ehs = (t.to(DEV) for t in _inputs())
    with pytest.raises(RuntimeError, match="prepare_training"):
        train_step(m32, DDPMScheduler(**SD_SCHED), None, lat, noi, torch.tensor([1, 2, 3]), ehs, cond)
    with pytest.raises(NotImplementedError):
        DDPMScheduler(**SD_SCHED).step(None, 0, None)
    # the reference script's --gradient_checkpointing call (train_brushnet_mirror.py:1153-1155) is accepted: recomputation is built (round 6)
    assert not m32.brushnet.gradient_checkpointing
    m32.brushnet.enable_gradient_checkpointing()
    assert m32.brushnet.gradient_checkpointing


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16x1"])
@pytest.mark.parametrize("train_unet", [False, True])
def test_gradient_checkpointing_recomputes_and_changes_nothing(prec, train_unet):
    """enable_gradient_checkpointing() (brushnet.py:674-676; the reference wraps every resnet / transformer of its blocks in
    torch.utils.checkpoint, unet_2d_blocks.py:1167-1196): each block's forward runs on a throw-away tape and again in the backward
    pass.  Two AdamW steps with changing inputs give bit-identical losses, gradient norms, gradients and weights with and without
    it; the tape of a checkpointed forward holds one closure per block instead of one per operator; and the checkpointed step
    keeps less memory alive between forward and backward."""
    from reflecting_reality_amd import autograd

    def run(ckpt):
        model = _model(prec).prepare_training(train_base_unet=train_unet)
        if ckpt:
            model.brushnet.enable_gradient_checkpointing()
            model.unet.enable_gradient_checkpointing()
        ns = DDPMScheduler(**SD_SCHED)
        opt = AdamW(model.get_trainable_modules(), lr=1e-5)
        out = []
        for lat, noi, ts, ehs, cond in _batches():
            loss, norm = train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV), max_grad_norm=1.0)
            out.append((float(loss), float(norm)))
        g = {k: v.clone() for m in model.get_trainable_modules() for k, v in m.grad_state_dict().items()}
        w = {k: v.clone() for m in model.get_trainable_modules() for k, v in m.state_dict().items()}
        return out, g, w

    calls = {"n": 0}
    real = autograd.checkpoint

    def counting(fn):
        calls["n"] += 1
        return real(fn)

    autograd.checkpoint = counting
    try:
        a_out, a_g, a_w = run(True)
    finally:
        autograd.checkpoint = real
    assert calls["n"] > 10, "no block went through autograd.checkpoint"
    b_out, b_g, b_w = run(False)
    print(f"[{prec}, train_unet={train_unet}] {calls['n']} checkpointed block forwards; (loss, norm) per step {a_out}")
    assert a_out == b_out
    for k in b_g:
        assert torch.equal(a_g[k], b_g[k]), f"gradient of {k} differs under checkpointing"
    for k in b_w:
        assert torch.equal(a_w[k], b_w[k]), f"weight {k} differs under checkpointing"


# ---- backward kernels one by one, against torch autograd on the CPU (float64) ----------------------------------------
def _rel(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


@pytest.mark.parametrize("code_name", ["fp32", "f16x3", "bf16x1"])
@pytest.mark.parametrize("case", ["3x3", "1x1", "s2p1", "s2asym", "up", "cat", "big"])
def test_conv_wgrad_and_dgrad(code_name, case):
    """mf_conv_wgrad and the data gradient (mf_gemm_conv on the transposed, tap-flipped weight; mf_zero_insert2x for
    stride 2, mf_sumpool2x2 behind the fused nearest-2x upsample) against torch autograd."""
    from reflecting_reality_amd import autograd as AG
    prec = ops.Precision.get(code_name)
    g = torch.Generator().manual_seed(51)
    b, cin, cout, h, w_ = (2, 24, 40, 10, 14) if case != "big" else (2, 320, 320, 32, 32)
    k = 1 if case == "1x1" else 3
    c1 = 16 if case == "cat" else 0
    x = torch.randn(b, cin, h, w_, generator=g, dtype=torch.float64)
    x1 = torch.randn(b, c1, h, w_, generator=g, dtype=torch.float64) if c1 else None
    wt = torch.randn(cout, cin + c1, k, k, generator=g, dtype=torch.float64) * 0.05
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    xs = [t.requires_grad_(True) for t in ([x, x1] if c1 else [x])]
    wt.requires_grad_(True); bias.requires_grad_(True)
    xin = torch.cat(xs, 1)
    kw = dict(stride=1, padding=1)
    if case == "1x1":
        ref = torch.nn.functional.conv2d(xin, wt, bias); kw = dict(stride=1, padding=0)
    elif case == "s2p1":
        ref = torch.nn.functional.conv2d(xin, wt, bias, stride=2, padding=1); kw = dict(stride=2, padding=1)
    elif case == "s2asym":
        ref = torch.nn.functional.conv2d(torch.nn.functional.pad(xin, (0, 1, 0, 1)), wt, bias, stride=2); kw = dict(stride=2, padding=(0, 0, 1, 1))
    elif case == "up":
        ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(xin, scale_factor=2.0, mode="nearest"), wt, bias, padding=1)
        kw = dict(stride=1, padding=1, upsample=True)
    else:
        ref = torch.nn.functional.conv2d(xin, wt, bias, padding=1)
    gy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(gy)

    class Holder:            # stands in for a model: owns the arenas' generation counter
        _weights_gen = 0
    cp = (cin + c1 + 3) // 4 * 4
    wk = torch.nn.functional.pad(wt.detach().float().permute(0, 2, 3, 1), (0, cp - cin - c1)).reshape(cout, k * k * cp).to(DEV).contiguous()
    p_w = AG.Param("w", wk, torch.zeros_like(wk))
    p_b = AG.Param("b", bias.detach().float().to(DEV), torch.zeros(cout, device=DEV))
    cw = ops.ConvWeight.from_params(p_w, p_b, prec, cout, cin + c1, cp, k, k, Holder())
    xa = x.detach().float().permute(0, 2, 3, 1).contiguous().to(DEV)
    x1a = x1.detach().float().permute(0, 2, 3, 1).contiguous().to(DEV) if c1 else None
    tape = AG.Tape(prec.tape_code)
    ops.TAPE = tape
    try:
        y = ops.conv2d(xa, cw, x1=x1a, **kw)
    finally:
        ops.TAPE = None
    # bf16x1: every operand is rounded to bf16 (2^-9 relative) before ONE MFMA per product, fp32 accumulate
    assert _rel(y.permute(0, 3, 1, 2), ref.detach()) < (1e-5 if code_name != "bf16x1" else 5e-3)
    tape.add(y, gy.float().permute(0, 2, 3, 1).contiguous().to(DEV))
    got = {}
    orig_add = tape.add
    tape.add = lambda t, gg: got.__setitem__(t.data_ptr(), gg) if t is not None else None
    tape.backward()
    tol = {"fp32": 1e-5, "f16x3": 3e-5, "bf16x1": 5e-3}[code_name]
    dw = p_w.grad.view(cout, k, k, cp)[..., : cin + c1].permute(0, 3, 1, 2)
    print(f"wgrad[{case},{code_name}] {_rel(dw, wt.grad):.2e}  dbias {_rel(p_b.grad, bias.grad):.2e}  dx {_rel(got[xa.data_ptr()].view(xa.shape).permute(0, 3, 1, 2), xs[0].grad):.2e}")
    assert _rel(dw, wt.grad) < tol and _rel(p_b.grad, bias.grad) < tol
    assert _rel(got[xa.data_ptr()].view(xa.shape).permute(0, 3, 1, 2), xs[0].grad) < tol
    if c1:
        assert _rel(got[x1a.data_ptr()].view(x1a.shape).permute(0, 3, 1, 2), xs[1].grad) < tol


def test_weight_gradient_on_bf16_inputs_lds_dma_equals_register_staged():
    """mf_conv_wgrad with bf16 x / dy (the bf16x1 mode's pre-rounded operands): the LDS-DMA kernel (three stages, chunks swizzled on
    the global side, zeros from the descriptor's range check) is bit-identical to the register-staged kernel it replaces, and both
    match float64 on the same bf16 values.  Shapes: 3x3 / 1x1 / stride 2 / asymmetric padding / fused upsample / two input segments
    (C0 % 128 == 0) / ragged N, C and pixel counts / a pixel split into several slabs."""
    g = torch.Generator().manual_seed(62)
    cases = [  # (b, h, w, c0, c1, n, k, stride, pad_t, pad_l, upsample)
        (2, 32, 32, 320, 0, 320, 3, 1, 1, 1, False), (8, 64, 64, 320, 0, 320, 3, 1, 1, 1, False), (2, 16, 16, 1280, 0, 640, 1, 1, 0, 0, False),
        (2, 33, 31, 136, 0, 72, 3, 1, 1, 1, False), (2, 32, 32, 320, 0, 640, 3, 2, 1, 1, False), (1, 17, 19, 64, 0, 200, 3, 2, 0, 0, False),
        (2, 8, 8, 256, 128, 384, 3, 1, 1, 1, False), (2, 16, 16, 128, 64, 96, 3, 1, 1, 1, True), (3, 5, 7, 8, 0, 8, 3, 1, 1, 1, False),
    ]
    for b, h, w_, c0, c1, n, k, stride, pt, pl, up in cases:
        hu, wu = (2 * h, 2 * w_) if up else (h, w_)
        ho = (hu + 2 * pt - k) // stride + 1 if (pt, pl) != (0, 0) or k == 1 else (hu + 1 - k) // stride + 1
        wo = (wu + 2 * pl - k) // stride + 1 if (pt, pl) != (0, 0) or k == 1 else (wu + 1 - k) // stride + 1
        x = torch.randn(b, h, w_, c0, generator=g).bfloat16().to(DEV)
        x1 = torch.randn(b, h, w_, c1, generator=g).bfloat16().to(DEV) if c1 else None
        dy = torch.randn(b * ho * wo, n, generator=g).bfloat16().to(DEV)
        res = []
        for dma in (True, False):
            hip.set_wgrad_dma(dma)
            try:
                dw = torch.full((n, k * k * (c0 + c1)), 0.5, device=DEV)
                hip.conv_wgrad(x, dy, dw, code=hip.MF_BF16, c0=c0, x1=x1, c1=c1, batch=b, h_in=h, w_in=w_, h_out=ho, w_out=wo, kh=k, kw=k,
                               stride=stride, pad_t=pt, pad_l=pl, upsample=up, n=n)
            finally:
                hip.set_wgrad_dma(True)
            res.append(dw)
        assert torch.equal(res[0], res[1]), (b, h, w_, c0, c1, n, k, stride, up)
        xin = torch.cat([x, x1], -1) if c1 else x
        xin = xin.double().permute(0, 3, 1, 2).cpu()
        if up:
            xin = torch.nn.functional.interpolate(xin, scale_factor=2.0, mode="nearest")
        wt = torch.zeros(n, c0 + c1, k, k, dtype=torch.float64, requires_grad=True)
        if (pt, pl) == (0, 0) and k == 3:
            ref = torch.nn.functional.conv2d(torch.nn.functional.pad(xin, (0, 1, 0, 1)), wt, stride=stride)
        else:
            ref = torch.nn.functional.conv2d(xin, wt, stride=stride, padding=(pt, pl))
        assert ref.shape[2:] == (ho, wo)
        ref.backward(dy.double().cpu().view(b, ho, wo, n).permute(0, 3, 1, 2))
        got = (res[0] - 0.5).view(n, k, k, c0 + c1).permute(0, 3, 1, 2)
        assert _rel(got, wt.grad) < 2e-5, (b, h, w_, c0, c1, n, k, stride, up)


def test_every_weight_gradient_form_of_the_plan_against_float64():
    """Each kernel form mf_conv_wgrad_plan names (0 fp32, 1 128-wide register-staged, 2 160-wide, 3 128-wide LDS-DMA), for every dtype
    that reaches it, on the smallest shape of tests/test_wgrad_plan_cpu.py's table that takes it, against conv2d's weight gradient in
    float64.  The form is asserted first: a change of routing cannot quietly shrink what this covers.  Bounds are the ones of the tests
    above: 1e-5 fp32, 3e-5 f16x3, 5e-3 bf16x1 on fp32 inputs (operands rounded to 2^-9), 2e-5 MF_BF16 against float64 on the same bf16 values."""
    from test_wgrad_plan_cpu import conv as plan_desc, planned
    g = torch.Generator().manual_seed(63)
    shapes = [  # (b, hw, c, n, k), [(dtype code, form, accumulate, bound)]
        ((4, 32, 320, 320, 3), [(hip.MF_F16X3, 2, 1, 3e-5), (hip.MF_BF16X1, 2, 1, 5e-3), (hip.MF_BF16, 2, 1, 2e-5)]),
        ((2, 16, 160, 160, 3), [(hip.MF_BF16X1, 1, 1, 5e-3), (hip.MF_BF16, 3, 1, 2e-5)]),
        ((2, 8, 64, 64, 3), [(hip.MF_F32, 0, 0, 1e-5), (hip.MF_F32, 0, 1, 1e-5)]),
    ]
    for (b, hw, c, n, k), runs in shapes:
        x, dy = torch.randn(b, hw, hw, c, generator=g), torch.randn(b * hw * hw, n, generator=g)
        refs = {}

        def ref_of(in16):          # float64 on the values the kernel is given: the fp32 tensors, or their bf16 roundings
            if in16 not in refs:
                xs, dys = (x.bfloat16(), dy.bfloat16()) if in16 else (x, dy)
                wt = torch.zeros(n, c, k, k, dtype=torch.float64, requires_grad=True)
                torch.nn.functional.conv2d(xs.double().permute(0, 3, 1, 2), wt, padding=k // 2).backward(dys.double().view(b, hw, hw, n).permute(0, 3, 1, 2))
                refs[in16] = wt.grad
            return refs[in16]

        for code, form, acc, bound in runs:
            p = planned(plan_desc(code, b, hw, hw, c, n, k, accumulate=acc))
            assert p.form == form, (code, b, hw, c, n, k, p.form)
            in16 = code == hip.MF_BF16
            xd, dyd = (t.bfloat16().to(DEV) if in16 else t.to(DEV) for t in (x, dy))
            dw = torch.full((n, k * k * c), 0.5, device=DEV)          # accumulate: += on 0.5; else overwritten
            hip.conv_wgrad(xd, dyd, dw, code=code, c0=c, batch=b, h_in=hw, w_in=hw, h_out=hw, w_out=hw, kh=k, kw=k, pad_t=k // 2, pad_l=k // 2,
                           n=n, accumulate=bool(acc))
            err = _rel((dw - 0.5 * acc).view(n, k, k, c).permute(0, 3, 1, 2), ref_of(in16))
            print(f"wgrad form {p.form} dtype {code} {b}x{hw}x{hw} {c}->{n} accumulate={acc} splitm={p.splitm} reduce={p.reduce_launch}: {err:.2e} (bound {bound:.0e})")
            assert err < bound, (code, form, acc, err)


@pytest.mark.parametrize("code_name", ["f16x3", "bf16x3"])
def test_device_split_pack_matches_the_host_split(code_name):
    """mf_split_pack (the per-step split of the weights the optimizer just changed) is bit-identical to ops.split_pack (the split the
    inference weights get once on the host), including the zero padding of K to whole 32-blocks and a strided source."""
    code = {"f16x3": hip.MF_F16X3, "bf16x3": hip.MF_BF16X3}[code_name]
    g = torch.Generator().manual_seed(61)
    for rows, k, ld in ((7, 36, 36), (320, 2880, 2880), (5, 31, 40), (64, 64, 64)):
        buf = (torch.randn(rows, ld, generator=g) * torch.logspace(-6, 2, ld)[None, :]).to(DEV)
        w = buf[:, :k]
        got, kp = hip.split_pack(w, code)
        ref, kp_ref = ops.split_pack(w.contiguous(), code)
        assert kp == kp_ref and got.shape == ref.shape and got.dtype == ref.dtype
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    if code == hip.MF_F16X3:
        hip.split_overflow(reset=True)
        big = torch.full((4, 32), 7.0e4, device=DEV)
        hip.split_pack(big, code)
        assert hip.split_overflow(reset=True) != 0


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("shape", [(2, 64, 0, 6, 10, 32), (2, 1280, 640, 8, 8, 32), (1, 320, 0, 64, 64, 32), (3, 32, 32, 5, 3, 16),
                                   (2, 1280, 1280, 16, 16, 32), (2, 320, 640, 32, 32, 32), (2, 640, 0, 17, 19, 32), (1, 64, 0, 40, 40, 32),
                                   (1, 320, 0, 64, 64, 32, "blocks")])
def test_groupnorm_backward(shape, silu):
    """hw >= 256 runs the streaming form (five launches, float4 over channels: 640 quads > 256 threads, 10 / 30 channels per group
    straddling quads, a ragged last pixel chunk, 16 pixel rows in flight); "blocks" withholds the workspace = the one-block-per-
    (image, group) kernel at the same size."""
    streaming = len(shape) == 6
    b, c0, c1, h, w_, groups = shape[:6]
    g = torch.Generator().manual_seed(52)
    x = (torch.randn(b, c0 + c1, h, w_, generator=g, dtype=torch.float64) * 1.7 + 0.3).requires_grad_(True)
    gamma = torch.randn(c0 + c1, generator=g, dtype=torch.float64).requires_grad_(True)
    beta = torch.randn(c0 + c1, generator=g, dtype=torch.float64).requires_grad_(True)
    y = torch.nn.functional.group_norm(x, groups, gamma, beta, 1e-5)
    y = torch.nn.functional.silu(y) if silu else y
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    xa = x.detach().float().permute(0, 2, 3, 1).contiguous().to(DEV)
    x0, x1 = (xa[..., :c0].contiguous(), xa[..., c0:].contiguous()) if c1 else (xa, None)
    dx0, dx1, dg, db = hip.groupnorm_bwd(x0, gy.float().permute(0, 2, 3, 1).contiguous().to(DEV), gamma.detach().float().to(DEV),
                                         beta.detach().float().to(DEV), groups=groups, eps=1e-5, silu=silu, x1=x1, streaming=streaming)
    dx = torch.cat([dx0, dx1], -1) if c1 else dx0
    e = (_rel(dx.permute(0, 3, 1, 2), x.grad), _rel(hip.colsum(dg, c0 + c1)[0], gamma.grad), _rel(hip.colsum(db, c0 + c1)[0], beta.grad))
    print(f"groupnorm_bwd{shape} silu={silu}: dx {e[0]:.2e} dgamma {e[1]:.2e} dbeta {e[2]:.2e}")
    assert max(e) < 2e-5
    if streaming and h * w_ >= 256:
        # the form the training tape uses: parameter gradients ADDED to the arena by the kernel (no partials, no colsum)
        acc = (torch.full((c0 + c1,), 0.5, device=DEV), torch.full((c0 + c1,), -0.25, device=DEV))
        dx0b, dx1b, dg2, db2 = hip.groupnorm_bwd(x0, gy.float().permute(0, 2, 3, 1).contiguous().to(DEV), gamma.detach().float().to(DEV),
                                                 beta.detach().float().to(DEV), groups=groups, eps=1e-5, silu=silu, x1=x1, grad_acc=acc)
        assert dg2 is None and db2 is None and torch.equal(dx0b, dx0)
        assert _rel(acc[0] - 0.5, gamma.grad) < 2e-5 and _rel(acc[1] + 0.25, beta.grad) < 2e-5
    # the (mean, rstd) the FORWARD kernel keeps (every forward path: slab / fused finalize / separate finalize) fed to the backward
    # pass, which then skips its statistics pass: the same gradients to fp32 rounding, and the statistics themselves against float64
    stats = torch.empty(b, groups, 2, device=DEV)
    hip.groupnorm(x0, gamma.detach().float().to(DEV), beta.detach().float().to(DEV), groups=groups, eps=1e-5, silu=silu,
                  out_dtype=torch.float32, x1=x1, stats_out=stats)
    xg = x.detach().view(b, groups, -1)
    assert _rel(stats[..., 0], xg.mean(-1)) < 2e-6 and _rel(stats[..., 1], 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-5)) < 2e-6
    sx0, sx1, sdg, sdb = hip.groupnorm_bwd(x0, gy.float().permute(0, 2, 3, 1).contiguous().to(DEV), gamma.detach().float().to(DEV),
                                           beta.detach().float().to(DEV), groups=groups, eps=1e-5, silu=silu, x1=x1, streaming=streaming,
                                           stats=stats)
    sdx = torch.cat([sx0, sx1], -1) if c1 else sx0
    assert max(_rel(sdx.permute(0, 3, 1, 2), x.grad), _rel(hip.colsum(sdg, c0 + c1)[0], gamma.grad), _rel(hip.colsum(sdb, c0 + c1)[0], beta.grad)) < 2e-5
    # dx = gradient + add (the gradient a residual connection already left): both kernel forms
    add0 = torch.randn_like(x0)
    add1 = torch.randn_like(x1) if c1 else None
    ex0, ex1, _, _ = hip.groupnorm_bwd(x0, gy.float().permute(0, 2, 3, 1).contiguous().to(DEV), gamma.detach().float().to(DEV),
                                       beta.detach().float().to(DEV), groups=groups, eps=1e-5, silu=silu, x1=x1, streaming=streaming,
                                       add0=add0, add1=add1)
    assert torch.allclose(ex0, dx0 + add0, rtol=0, atol=2e-6 * float(dx0.abs().max() + add0.abs().max()))
    if c1:
        assert torch.allclose(ex1, dx1 + add1, rtol=0, atol=2e-6 * float(dx1.abs().max() + add1.abs().max()))


def test_layernorm_softmax_geglu_silu_backward():
    g = torch.Generator().manual_seed(53)
    for rows, c in ((130, 320), (64, 1280), (5, 32), (4100, 320), (1000, 640), (300, 2048), (77, 96), (70000, 64)):
        x = torch.randn(rows, c, generator=g, dtype=torch.float64).requires_grad_(True)
        gamma = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_(True)
        beta = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_(True)
        y = torch.nn.functional.layer_norm(x, (c,), gamma, beta, 1e-5)
        gy = torch.randn(rows, c, generator=g, dtype=torch.float64)
        y.backward(gy)
        dx, dg, db = hip.layernorm_bwd(x.detach().float().to(DEV), gy.float().to(DEV), gamma.detach().float().to(DEV), 1e-5)
        ad = torch.randn(rows, c, generator=g).to(DEV)
        dxa, _, _ = hip.layernorm_bwd(x.detach().float().to(DEV), gy.float().to(DEV), gamma.detach().float().to(DEV), 1e-5, add=ad)
        assert torch.allclose(dxa, dx + ad, rtol=0, atol=2e-6 * float(dx.abs().max() + ad.abs().max()))
        e = (_rel(dx, x.grad), _rel(hip.colsum(dg, c)[0], gamma.grad), _rel(hip.colsum(db, c)[0], beta.grad))
        print(f"layernorm_bwd {rows}x{c}: {e}")
        assert max(e) < 2e-5
    s = torch.randn(37, 80, generator=g, dtype=torch.float64).requires_grad_(True)
    p = torch.softmax(s[:, :77] * 0.3, -1)
    gp = torch.randn(37, 77, generator=g, dtype=torch.float64)
    p.backward(gp)
    pp = torch.zeros(37, 80); pp[:, :77] = p.detach().float()
    dp = torch.zeros(37, 80); dp[:, :77] = gp.float()
    ds = hip.softmax_bwd(pp.to(DEV), dp.to(DEV), 77, 0.3)
    assert _rel(ds[:, :77], s.grad[:, :77]) < 2e-5 and float(ds[:, 77:].abs().max()) == 0.0
    hh = torch.randn(50, 2 * 96, generator=g, dtype=torch.float64).requires_grad_(True)
    a, gt = hh.chunk(2, -1)
    out = a * torch.nn.functional.gelu(gt)
    go = torch.randn(50, 96, generator=g, dtype=torch.float64)
    out.backward(go)
    assert _rel(hip.geglu_bwd(hh.detach().float().to(DEV), go.float().to(DEV)), hh.grad) < 2e-5
    z = torch.randn(1000, generator=g, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.silu(z).backward(torch.ones(1000, dtype=torch.float64))
    assert _rel(hip.silu_bwd(z.detach().float().to(DEV), torch.ones(1000, device=DEV)), z.grad) < 2e-5


@pytest.mark.parametrize("code_name", ["fp32", "f16x3"])
@pytest.mark.parametrize("heads,d,sq,skv", [(2, 40, 96, 96), (4, 8, 64, 77), (8, 40, 1024, 1024), (2, 40, 4096, 4096), (4, 40, 1024, 77),
                                            (3, 8, 260, 300)])
def test_attention_backward(code_name, heads, d, sq, skv):
    """f16x3 with >= 256 queries and head dim 8 / 40 runs the FLASH backward (mf_attention_bwd_f16x3: two passes of one kernel
    that recompute P from the forward's row statistics); everything else the unfused one.  Both against torch autograd in
    float64."""
    from reflecting_reality_amd import autograd as AG
    prec = ops.Precision.get(code_name)
    g = torch.Generator().manual_seed(54)
    c = heads * d
    q, k, v = (torch.randn(2, s_, c, generator=g, dtype=torch.float64).requires_grad_(True) for s_ in (sq, skv, skv))
    qh, kh, vh = (t.view(2, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    o = (torch.softmax(qh @ kh.transpose(-1, -2) / d ** 0.5, -1) @ vh).transpose(1, 2).reshape(2, sq, c)
    go = torch.randn(2, sq, c, generator=g, dtype=torch.float64)
    o.backward(go)
    qd, kd, vd = (t.detach().float().to(DEV) for t in (q, k, v))
    tape = AG.Tape(prec.code if prec.split else 0)
    ops.TAPE = tape
    try:
        out = ops.attention_train(qd, kd, vd, heads, 1.0 / d ** 0.5, prec)
    finally:
        ops.TAPE = None
    assert _rel(out, o.detach()) < 2e-5
    tape.add(out, go.float().to(DEV))
    got = {}
    tape.add = lambda t, gg: got.__setitem__(t.data_ptr(), gg)
    tape.backward()
    e = [_rel(got[t.data_ptr()].view(t.shape), r.grad) for t, r in ((qd, q), (kd, k), (vd, v))]
    flash = code_name == "f16x3" and d in ops.FLASH_BWD_HEAD_DIMS and sq >= ops.FLASH_BWD_MIN_TOKENS and sq % 4 == 0
    print(f"attention backward[{code_name}, h{heads} d{d} {sq}x{skv}, {'flash' if flash else 'unfused'}]: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < 3e-5


@pytest.mark.parametrize("heads,d,sq,skv", [(8, 40, 1024, 1024), (2, 40, 4096, 4096), (4, 40, 1024, 77), (3, 8, 260, 300), (2, 8, 256, 77),
                                            (8, 80, 1024, 1024), (8, 80, 1024, 77), (2, 80, 300, 333)])
def test_attention_backward_bf16_planes(heads, d, sq, skv):
    """The bf16x1 mode's attention on pre-rounded operands (mf_attention_bf16_lse + mf_attention_bwd_bf16): against torch autograd
    in float64 ON THE bf16-ROUNDED q / k / v / dO — what the reference's bf16 autocast feeds F.scaled_dot_product_attention —
    so the difference is the kernel's own roundings: of q * scale * log2(e) in the forward (the inference kernel folds the scale into
    its Q tile — one rounding the reference does not have, the size of the input rounding itself), of P / dS, and of the bf16
    output.  Bound 1e-2 of the tensor's maximum (bf16 has 8 bits: 2^-9 = 2e-3 per rounding; measured 2e-3 .. 7e-3)."""
    from reflecting_reality_amd import autograd as AG
    prec = ops.Precision.get("bf16x1")
    assert ops.BF16X1_FAST
    g = torch.Generator().manual_seed(57)
    c = heads * d
    r16 = lambda t: t.float().bfloat16().double()
    q, k, v = (r16(torch.randn(2, s_, c, generator=g, dtype=torch.float64)).requires_grad_(True) for s_ in (sq, skv, skv))
    qh, kh, vh = (t.view(2, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    o = (torch.softmax(qh @ kh.transpose(-1, -2) / d ** 0.5, -1) @ vh).transpose(1, 2).reshape(2, sq, c)
    go = r16(torch.randn(2, sq, c, generator=g, dtype=torch.float64))
    o.backward(go)
    qd, kd, vd = (t.detach().float().to(DEV) for t in (q, k, v))
    tape = AG.Tape(prec.code)
    ops.TAPE = tape
    try:
        out = ops.attention_train(qd, kd, vd, heads, 1.0 / d ** 0.5, prec)
    finally:
        ops.TAPE = None
    assert out.dtype == torch.bfloat16                   # the flash path ran
    assert _rel(out.float(), o.detach()) < 1e-2
    tape.add(out, go.float().to(DEV))
    got = {}
    tape.add = lambda t, gg: got.__setitem__(t.data_ptr(), gg)
    tape.backward()
    e = [_rel(got[t.data_ptr()].view(t.shape), r.grad) for t, r in ((qd, q), (kd, k), (vd, v))]
    print(f"attention backward[bf16 planes, h{heads} d{d} {sq}x{skv}]: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}")
    assert max(e) < 1e-2


def test_bf16_tensors_of_the_bf16x1_mode_geglu_transpose_attention_outputs():
    """The tensors the bf16x1 mode keeps in bf16 (q / k / v, FeedForward's pre-activation) and their gradients:
    mf_geglu (bf16 -> bf16, vectorised) and mf_geglu_bwd_bf16 (+ the bias gradient from the same pass) against float64 on the rounded
    inputs; mf_transpose_bf16_bf16 exact; the attention backward's bf16 outputs = its fp32 outputs rounded (same kernel)."""
    from reflecting_reality_amd import autograd as AG
    g = torch.Generator().manual_seed(59)
    for rows, c in ((4096, 1280), (77, 2560), (1000, 5120), (5, 16), (300, 648)):
        h = torch.randn(rows, 2 * c, generator=g).bfloat16()
        do = torch.randn(rows, c, generator=g)
        hd = h.double().requires_grad_(True)
        a, gt = hd.chunk(2, -1)
        out = a * torch.nn.functional.gelu(gt)
        out.backward(do.double())
        got = hip.geglu(h.to(DEV), torch.bfloat16)
        assert _rel(got.float(), out.detach()) < 4e-3                      # one bf16 rounding of the output
        bias0 = torch.randn(2 * c, generator=g)
        bias = bias0.clone().to(DEV)
        dh = hip.geglu_bwd_bf16(h.to(DEV), do.to(DEV), bias)
        assert dh.dtype == torch.bfloat16 and _rel(dh.float(), hd.grad) < 4e-3
        # the bias gradient is the column sum of the ROUNDED gradient tensor
        ref_b = dh.double().sum(0).cpu()
        assert float((bias.cpu().double() - bias0.double() - ref_b).abs().max()) < 2e-5 * float(dh.double().abs().sum(0).max()) + 1e-6
        assert torch.equal(hip.geglu_bwd_bf16(h.to(DEV), do.to(DEV)), dh)
    for nz, rows, cols in ((2, 4096, 320), (3, 77, 640), (1, 1024, 1280), (2, 260, 24), (1, 8, 8)):
        x = torch.randn(nz, rows, cols, generator=g).bfloat16().to(DEV)
        ld = (rows + 7) // 8 * 8
        y = torch.full((nz, cols, ld), 7.0, dtype=torch.bfloat16, device=DEV)
        hip.transpose(x, rows, cols, nz=nz, ldx=cols, ldy=ld, zsx=rows * cols, zsy=cols * ld, out=y)
        assert torch.equal(y[:, :, :rows], x.transpose(1, 2)) and float(y[:, :, rows:].abs().max() if ld > rows else 0.0) == 0.0
    # fp32 -> bf16 transposes: the vectorised form (and the scalar fallback at odd sizes) against torch; the data-gradient weight
    # layout (taps flipped by a negative batch stride, as autograd._dgrad_weight calls it)
    for nz, rows, cols in ((2, 4096, 320), (3, 77, 640), (1, 1000, 1284), (2, 33, 24), (1, 36, 7)):
        x = torch.randn(nz, rows, cols, generator=g).to(DEV)
        ld = (rows + 7) // 8 * 8
        y = torch.zeros(nz, cols, ld, dtype=torch.bfloat16, device=DEV)
        hip.transpose(x, rows, cols, nz=nz, ldx=cols, ldy=ld, zsx=rows * cols, zsy=cols * ld, out=y)
        assert torch.equal(y[:, :, :rows], x.transpose(1, 2).bfloat16()) and float(y[:, :, rows:].float().abs().max() if ld > rows else 0.0) == 0.0
    n, ct, taps = 320, 640, 9
    w = torch.randn(n, taps * ct, generator=g).to(DEV)
    wd = torch.zeros(ct, taps * n, dtype=torch.bfloat16, device=DEV)
    hip.transpose(w, n, ct, nz=taps, ldx=taps * ct, ldy=taps * n, zsx=ct, zsy=-n, out=wd, y_offset=(taps - 1) * n)
    ref = w.view(n, taps, ct).flip(1).permute(2, 1, 0).reshape(ct, taps * n).bfloat16()
    assert torch.equal(wd, ref)
    prec = ops.Precision.get("bf16x1")
    for heads, d, sq, skv in ((8, 40, 1024, 1024), (4, 80, 512, 77), (2, 8, 256, 300)):
        c = heads * d
        q, k, v = (torch.randn(2, s_, c, generator=g).bfloat16().to(DEV) for s_ in (sq, skv, skv))
        go = torch.randn(2, sq, c, generator=g).to(DEV)
        res = []
        for cast in (lambda t: t, lambda t: t.float()):
            tape = AG.Tape(prec.code)
            ops.TAPE = tape
            try:
                qq, kk, vv = cast(q), cast(k), cast(v)
                out = ops.attention_train(qq, kk, vv, heads, 1.0 / d ** 0.5, prec)
            finally:
                ops.TAPE = None
            tape.add(out, go)
            got = {}
            tape.add = lambda t, gg: got.__setitem__(t.data_ptr(), gg)
            tape.backward()
            res.append((out, [got[t.data_ptr()] for t in (qq, kk, vv)]))
        assert torch.equal(res[0][0], res[1][0])
        for a16, a32 in zip(res[0][1], res[1][1]):
            assert a16.dtype == torch.bfloat16 and a32.dtype == torch.float32 and torch.equal(a16.view(-1), a32.view(-1).bfloat16())


def test_cast_bf16_with_column_sums_in_one_read():
    """mf_cast_bf16_colsum: the bf16 copy is bit-identical to mf_cast_bf16 / torch's rounding; the per-segment and total column sums
    match float64 sums to fp32 accumulation error and are ADDED to what the targets held."""
    g = torch.Generator().manual_seed(58)
    for segs, rps, n, ldo in ((8, 4096, 320, 1280), (1, 32768, 320, 320), (8, 64, 1280, 1280), (2, 77, 8, 16), (3, 5, 2560, 2560),
                              (8, 1024, 640, 640), (1, 1, 24, 24), (4, 300, 1928, 2000)):
        x = torch.randn(segs * rps, n, generator=g) * 3.0 + 0.25
        xd = x.to(DEV)
        seg0, tot0 = torch.randn(segs, ldo, generator=g), torch.randn(n, generator=g)
        seg, tot = seg0.clone().to(DEV), tot0.clone().to(DEV)
        out = hip.cast_bf16_colsum(xd, n, segs=segs, seg_out=seg, ldo=ldo, tot_out=tot)
        assert torch.equal(out.cpu(), x.bfloat16()) and torch.equal(out, hip.cast_bf16(xd))
        ref_seg = x.double().view(segs, rps, n).sum(1)
        scale = float(x.abs().double().view(segs, rps, n).sum(1).max())
        assert float((seg.cpu()[:, :n].double() - seg0[:, :n].double() - ref_seg).abs().max()) < 4e-6 * scale
        assert torch.equal(seg.cpu()[:, n:], seg0[:, n:])
        assert float((tot.cpu().double() - tot0.double() - ref_seg.sum(0)).abs().max()) < 4e-6 * scale * segs
        only_tot = torch.zeros(n, device=DEV)
        out2 = hip.cast_bf16_colsum(xd, n, tot_out=only_tot)
        assert torch.equal(out2, out) and float((only_tot.cpu().double() - ref_seg.sum(0)).abs().max()) < 4e-6 * scale * segs


def test_adamw_and_clip_against_torch():
    g = torch.Generator().manual_seed(55)
    n = 100003
    w = torch.randn(n, generator=g)
    pt = torch.nn.Parameter(w.clone())
    opt = torch.optim.AdamW([pt], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    wd, m, v = w.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
    coef, norm = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g) * (3.0 if step == 2 else 0.001)
        pt.grad = gr.clone()
        tn = torch.nn.utils.clip_grad_norm_([pt], 1.0)
        opt.step()
        gd = gr.to(DEV)
        hip.sumsq(gd, sumsq)
        hip.sumsq(gd * 1024.0, sumsq)                    # an arena holding gradients x 1024 (loss scale)
        hip.clip_coef(sumsq, 1.0, coef, norm, unscale=1.0 / 1024.0)
        assert abs(float(norm) - float(tn)) < 1e-5 * float(tn)
        hip.adamw(wd, gd * 1024.0, m, v, lr=1e-3, step=step, grad_scale=coef)
        assert float((wd.cpu() - pt.detach()).abs().max()) < 2e-6


DDP_WORKER = r"""
import json, os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import torch
from oracle import mirrorfusion_ref as R
from reflecting_reality_amd import DDPMScheduler, models as M, synth, distributed as D
from reflecting_reality_amd.training import AdamW, MirrorFusionModel, train_step
from util import keys
rank, world, _ = D.init_process_group("gloo")
DEV = "cuda"
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
def model():
    unet = M.UNet2DConditionModel(dict(R.TINY_UNET), precision="fp32", device=DEV)
    unet.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    bn = M.BrushNetModel(dict(R.brushnet_config(R.TINY_UNET, 5)), precision="fp32", device=DEV)
    bn.load_state_dict(synth.state_dict_for(keys("tiny_train")["brushnet"], 21))
    return MirrorFusionModel(unet, bn).prepare_training()
g = torch.Generator().manual_seed(77)
full = [torch.randn(6, 4, 8, 8, generator=g) * 0.8, torch.randn(6, 4, 8, 8, generator=g), torch.tensor([17, 480, 965, 702, 3, 250]),
        torch.randn(6, 77, 32, generator=g), torch.randn(6, 5, 8, 8, generator=g)]
ns = DDPMScheduler(**SD)
m = model()
opt = AdamW(m.get_trainable_modules())
sync = D.GradBuckets(m.get_trainable_modules(), bucket_floats=20000)      # ~25 buckets on the tiny BrushNet
sl = slice(3 * rank, 3 * rank + 3)
lat, noi, ts, ehs, cond = (t[sl] for t in full)
losses = []
for step in range(2):
    loss, norm = train_step(m, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV), grad_sync=sync)
    losses.append(D.gather_mean(loss))
sd = m.brushnet.state_dict()
out = dict(rank=rank, losses=losses, norm=float(norm))
if rank == 0:
    # the same two steps in ONE process on the concatenated batch: mean loss over 6 = mean of the ranks' mean losses
    m1 = model()
    o1 = AdamW(m1.get_trainable_modules())
    l1 = []
    for step in range(2):
        loss1, norm1 = train_step(m1, ns, o1, *(t.to(DEV) if i != 2 else t for i, t in enumerate(full)))
        l1.append(float(loss1))
    sd1 = m1.brushnet.state_dict()
    out["single_losses"], out["single_norm"] = l1, float(norm1)
    # Adam's step is ~lr * sign(g): compare the MOVEMENT of every tensor, and the weights themselves where gradients are not ~0
    w0 = synth.state_dict_for(keys("tiny_train")["brushnet"], 21)
    out["max_dw_rel"] = max(float(((sd[k] - w0[k]).norm() - (sd1[k] - w0[k]).norm()).abs() / ((sd1[k] - w0[k]).norm() + 1e-12)) for k in sd)
    out["max_w_diff"] = max(float((sd[k] - sd1[k]).abs().max()) for k in sd)
torch.save({k: v for k, v in sd.items()}, os.path.join(os.environ["RESULT_DIR"], f"w{rank}.pt"))
with open(os.path.join(os.environ["RESULT_DIR"], f"ddp{rank}.json"), "w") as f:
    json.dump(out, f)
"""


def test_data_parallel_training_two_ranks_equal_one_process_on_the_joint_batch(tmp_path):
    """(e) training: two ranks (sharing this GPU; gloo for the exchange, staged through the host) each train on half of
    a batch with the bucketed gradient all-reduce hooked into the backward tape; every rank ends with the same weights, and
    they match ONE process training on the joint batch (mean loss over 6 samples = mean of the two ranks' means)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "ddp_worker.py"
    script.write_text(DDP_WORKER % (root, root))
    from reflecting_reality_amd.distributed import torchrun_argv          # rendezvous on a port the store binds itself
    env = dict(os.environ, RESULT_DIR=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(torchrun_argv(2) + [str(script)], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    r0, r1 = (json.load(open(tmp_path / f"ddp{r}.json")) for r in range(2))
    w0, w1 = (torch.load(tmp_path / f"w{r}.pt") for r in range(2))
    for k in w0:
        assert torch.equal(w0[k], w1[k]), f"{k}: the two ranks diverged"
    print(r0)
    assert r0["losses"] == r1["losses"]
    for a, b in zip(r0["losses"], r0["single_losses"]):
        assert abs(a - b) < 2e-6 * abs(b)
    assert abs(r0["norm"] - r0["single_norm"]) < 1e-4 * r0["single_norm"]
    assert r0["max_w_diff"] < 3e-5       # 2 steps x lr 1e-5: a flipped near-zero gradient could move a weight by 2e-5 (measured 2e-6)


@pytest.mark.parametrize("train_unet,b", [(False, 8), (True, 4)])
def test_baseline_config3_full_size_step_determinism_and_forced_rccl_sync(train_unet, b, tmp_path):
    """BASELINE.json configs[3] at its own size: the MirrorFusion fine-tune step at per-GPU batch 8 x 512 x 512 (64 x 64 latents),
    full-size SD1.5 UNet (frozen) + BrushNet (trainable), f16x3 contractions, clip 1.0, AdamW (train_brushnet_mirror.py:1407-1466).
    No reference gradient exists at this size (the reference's autograd on the CPU would take hours), so the step is pinned by
    size-independent properties: (1) finite loss / gradient norm, every trainable tensor moves; (2) two identical runs are
    BIT-identical (fixed-order reductions, no atomics); (3) the same step with the bucketed gradient all-reduce forced through
    RCCL on this single rank (MF_FORCE_GRAD_SYNC=1: world size 1, sum of one = identity, divide by 1) is bit-identical to the
    unsynchronised step — the DDP path of distributed.GradBuckets changes nothing but the exchange.
    train_unet=True is --train_base_unet (train_brushnet_mirror.py:1073-1075) at full size: both nets train (batch 4 here; the
    exchange then carries both gradient arenas, 2.48 + 3.44 GB), and the UNet's weights must move too."""
    import torch.distributed as dist
    from reflecting_reality_amd import distributed as D
    from reflecting_reality_amd.configs import SD15_UNET, brushnet_config

    def build():
        unet = M.UNet2DConditionModel(dict(SD15_UNET), precision="f16x3", device=DEV)
        unet.load_state_dict(synth.state_dict_for(unet.param_shapes(), 0))
        bn = M.BrushNetModel(dict(brushnet_config(SD15_UNET, 6)), precision="f16x3", device=DEV)
        bn.load_state_dict(synth.state_dict_for(bn.param_shapes(), 1))
        return MirrorFusionModel(unet, bn).prepare_training(train_base_unet=train_unet)

    g = torch.Generator().manual_seed(303)
    lat, noi = torch.randn(b, 4, 64, 64, generator=g).to(DEV) * 0.8, torch.randn(b, 4, 64, 64, generator=g).to(DEV)
    cond, ehs = torch.randn(b, 6, 64, 64, generator=g).to(DEV), torch.randn(b, 77, 768, generator=g).to(DEV)
    ts = torch.tensor([981, 3, 500, 250, 751, 17, 640, 111])[:b]
    ns = DDPMScheduler(**SD_SCHED)

    def run(sync_factory=None):
        model = build()
        w0 = model.brushnet.flat_w.clone()
        u0 = model.unet.flat_w[: model.unet.num_arena_floats()].clone() if train_unet else None
        opt = AdamW(model.get_trainable_modules(), lr=1e-5)
        sync = sync_factory(model) if sync_factory else None
        out = []
        for _ in range(2):
            loss, norm = train_step(model, ns, opt, lat, noi, ts, ehs, cond, max_grad_norm=1.0, grad_sync=sync)
            out.append((float(loss), float(norm)))
        w = model.brushnet.flat_w.clone()
        n_used = model.brushnet.num_arena_floats()
        if train_unet:          # the UNet's arena trains too: fold a digest of it into the comparison
            u = model.unet.flat_w[: model.unet.num_arena_floats()]
            out.append((float(u.double().sum()), float((u.double() ** 2).sum())))
            assert (u != u0).float().mean().item() > 0.99, "the UNet's weights did not move under --train_base_unet"
            assert model.unet.flat_g is not None and len(model.get_trainable_modules()) == 2
        del model, opt
        torch.cuda.empty_cache()
        return out, w, w0, n_used

    a_out, a_w, w0, n_used = run()
    print(f"configs[3] step at batch {b} x 512^2 (train_base_unet={train_unet}): (loss, grad norm) per step", a_out)
    assert all(np.isfinite(v) for pair in a_out for v in pair) and a_out[0][1] > 0
    moved = (a_w[:n_used] != w0[:n_used]).float().mean().item()
    assert moved > 0.99, f"only {moved:.3f} of the trainable floats moved"
    b_out, b_w, _, _ = run()
    assert a_out == b_out and torch.equal(a_w, b_w), "two identical training runs must be bit-identical"

    os.environ["MF_FORCE_GRAD_SYNC"] = "1"
    # a file store: no port to probe, release and lose to another process (EADDRINUSE on the driver's box in round 5)
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdzv_store", rank=0, world_size=1)
    try:
        def factory(model):
            s = D.GradBuckets(model.get_trainable_modules())
            assert s.force and s.world == 1
            return s
        c_out, c_w, _, _ = run(factory)
    finally:
        dist.destroy_process_group()
        os.environ.pop("MF_FORCE_GRAD_SYNC", None)
    assert c_out == a_out and torch.equal(c_w, a_w), "the forced single-rank RCCL exchange changed the step"


def test_bench_train_under_torchrun_with_rccl_reports_all_reduce():
    """bench.py --mode train launched the way the driver launches N > 1 (python -m torch.distributed.run ... bench.py --gpus N)
    with the default backend (RCCL) and MF_FORCE_GRAD_SYNC=1 on this one GPU: the rendezvous, the bucketed exchange under
    the backward pass and time_all_reduce() (a --full measurement) all run over RCCL, and the JSON line carries all_reduce.ms."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from reflecting_reality_amd.distributed import torchrun_argv
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MF_BENCH_BACKEND")}
    env["MF_FORCE_GRAD_SYNC"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run(torchrun_argv(1) + [os.path.join(root, "bench.py"), "--gpus", "1", "--mode", "train", "--steps", "1",
                                             "--warmup", "1", "--batch", "2", "--size", "256", "--full"], capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 1 and rec["unit"] == "samples/sec" and rec["value"] > 0
    ar = rec["all_reduce"]
    assert ar is not None and ar["ms"] > 0 and ar["bytes"] > 1e9, ar
    print("single-rank RCCL all-reduce of the BrushNet gradient arena:", ar)


# ---- round 4: range guard over the WHOLE step, capture after a skipped warm-up, accumulation, lr schedule ---------------
def _skip_inputs(i, overflow=False):
    lat, noi, ts, ehs, cond = _batches()[i % 2]
    ts = (ts + 37 * i) % 1000
    ehs = ehs * (3.0e6 if overflow else 1.0)        # the UNet's to_k / to_v operands leave the fp16 range IN THE FORWARD pass
    return lat.to(DEV) * (1.0 + 0.1 * i), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV)


@pytest.mark.parametrize("graphed", [False, True])
def test_forward_overflow_skips_the_optimizer_step(graphed):
    """an f16x3 operand above 65504 in the FORWARD pass must skip the step (v_cvt_pkrtz saturates silently).  The
    guard flags are reset before the forward pass and read after the backward pass, in train_step and in GraphedTrainStep."""
    import warnings
    from reflecting_reality_amd.training import GraphedTrainStep
    ns = DDPMScheduler(**SD_SCHED)
    model = _model("f16x3").prepare_training()
    opt = AdamW(model.get_trainable_modules())
    step = GraphedTrainStep(model, ns, opt, warmup=1) if graphed else (lambda *a: train_step(model, ns, opt, *a))
    for i in range(2):                                # (graphed: one eager warm-up, then the capture)
        step(*_skip_inputs(i))
    w = model.brushnet.flat_w.clone()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        step(*_skip_inputs(2, overflow=True))
    assert any("exceeded the fp16 range" in str(r.message) for r in rec), "the overflowing step was not reported"
    assert torch.equal(model.brushnet.flat_w, w), "weights moved although a forward operand left the fp16 range"
    assert opt.step_count == 2 and getattr(model, "overflow_steps", 0) == 1
    step(*_skip_inputs(3))                            # and training goes on
    assert opt.step_count == 3 and not torch.equal(model.brushnet.flat_w, w)


def test_bf16x1_guard_arms_itself_when_the_shapes_start_using_fp16_halves(monkeypatch):
    """the bf16x1 guard was armed from the PREVIOUS step's count of fp16-split attention launches; a step that launches
    them after a step that launched none (the resolution changed) must still read the flags and skip a saturated step."""
    import warnings
    # the tiny model's 64-token, d = 8 attention on the route the full-size model's short sequences take with MFHIP_NO_FLASH_BWD's twin off
    monkeypatch.setattr(ops, "FLASH_BWD_MIN_TOKENS", 16)
    monkeypatch.setattr(ops, "FLASH_BWD_BF16_HEAD_DIMS", ())
    ns = DDPMScheduler(**SD_SCHED)
    model = _model("bf16x1").prepare_training()
    opt = AdamW(model.get_trainable_modules())
    train_step(model, ns, opt, *_skip_inputs(0))
    assert model._split_kernels_per_step > 0, "the test model's short sequences should run the fp16-split attention"
    model._split_kernels_per_step = 0                 # as if the previous step's shapes had all taken the bf16 flash route
    w = model.brushnet.flat_w.clone()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        train_step(model, ns, opt, *_skip_inputs(1, overflow=True))
    assert any("exceeded the fp16 range" in str(r.message) for r in rec), "the overflowing step was not reported"
    assert torch.equal(model.brushnet.flat_w, w) and model._split_kernels_per_step > 0


def test_flag_raised_between_forward_and_backward_counts(monkeypatch):
    """The discriminating form of the test above: a range-guard flag raised after the forward pass and before the backward pass
    (here by an unrelated overflowing split issued from the loss-gradient call) must still be set when train_step reads the
    flags — round 3's train_step cleared them at exactly that point."""
    import warnings
    ns = DDPMScheduler(**SD_SCHED)
    model = _model("f16x3").prepare_training()
    opt = AdamW(model.get_trainable_modules())
    orig = hip.mse_grad

    def mse_grad_and_overflow(*a, **k):
        hip.split_halves(torch.full((64,), 1.0e6, device=DEV))
        return orig(*a, **k)

    monkeypatch.setattr(hip, "mse_grad", mse_grad_and_overflow)
    w = model.brushnet.flat_w.clone()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        train_step(model, ns, opt, *_skip_inputs(0))
    assert any("exceeded the fp16 range" in str(r.message) for r in rec)
    assert torch.equal(model.brushnet.flat_w, w) and opt.step_count == 0


def test_capture_after_an_overflow_skipped_warmup_replays_on_live_weights():
    """when the warm-up step of GraphedTrainStep is skipped by the range guard the weight generation does not move,
    so the per-step re-layouts (split-pack of the forward weights, transpose + split-pack of the data-gradient weights) used to
    be left OUT of the captured graph, and every replay ran on frozen copies while AdamW kept updating the arena.  The capture
    now forces them in: the graphed run equals the eager run bit for bit over three optimizer steps after the skipped one."""
    import warnings
    from reflecting_reality_amd.training import GraphedTrainStep
    ns = DDPMScheduler(**SD_SCHED)

    def run(graphed):
        model = _model("f16x3").prepare_training()
        opt = AdamW(model.get_trainable_modules())
        step = GraphedTrainStep(model, ns, opt, warmup=1) if graphed else (lambda *a: train_step(model, ns, opt, *a))
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            step(*_skip_inputs(0, overflow=True))     # the warm-up call: skipped
            assert opt.step_count == 0
            for i in range(1, 5):
                loss, norm = step(*_skip_inputs(i))
                out.append((float(loss), float(norm)))
        assert opt.step_count == 4
        return model.brushnet.flat_w.clone(), out

    (wa, la), (wb, lb) = run(False), run(True)
    assert la == lb, (la, lb)
    assert torch.equal(wa, wb), "the graph captured after a skipped warm-up step trains on stale weight layouts"


def test_graphed_step_recaptures_when_the_arenas_move():
    """prepare_training() rebuilds the arenas: a graph captured before it points at freed memory and must not be replayed."""
    from reflecting_reality_amd.training import GraphedTrainStep
    ns = DDPMScheduler(**SD_SCHED)
    model = _model("fp32").prepare_training()
    opt = AdamW(model.get_trainable_modules())
    step = GraphedTrainStep(model, ns, opt, warmup=1)
    for i in range(3):
        step(*_skip_inputs(i))
    g0, key0 = step.graph, step._arena_key
    keep = (model.brushnet.flat_w, model.brushnet.flat_g)          # keep the old arenas alive so the new ones get new addresses
    model.prepare_training()
    opt2 = AdamW(model.get_trainable_modules())
    step.opt = opt2
    loss, norm = step(*_skip_inputs(3))
    assert step.graph is not g0 and step._arena_key != key0 and np.isfinite(float(loss)) and float(norm) > 0
    del keep


def test_gradient_accumulation_equals_the_joint_batch_and_the_lr_schedule_steps_with_the_optimizer():
    """--gradient_accumulation_steps 2 (train_brushnet_mirror.py:474-478, :1349): two calls on 3 samples each leave the
    gradients — and, after AdamW, the weights — of ONE call on the 6 samples (mean loss over 6 = mean of the two means; each
    micro-loss scaled by 1 / 2); the first call returns no norm, takes no optimizer step and leaves the schedule alone.  The
    schedule is optimization.get_scheduler's (pinned to the reference in tests/test_host_logic.py)."""
    from reflecting_reality_amd.optimization import get_scheduler
    ns = DDPMScheduler(**SD_SCHED)
    (l0, n0, t0, e0, c0), (l1, n1, t1, e1, c1) = _batches()

    model = _model("fp32").prepare_training()
    opt = AdamW(model.get_trainable_modules(), lr=1e-5)
    sch = get_scheduler("constant_with_warmup", opt, num_warmup_steps=2)
    assert opt.lr == 0.0
    sch.step()                                        # leave the zero-lr first step of the warm-up behind: lr = 5e-6
    loss_a, norm_a = train_step(model, ns, opt, l0.to(DEV), n0.to(DEV), t0, e0.to(DEV), c0.to(DEV), gradient_accumulation_steps=2,
                                lr_scheduler=sch)
    assert norm_a is None and opt.step_count == 0 and opt.lr == 5e-6 and opt._micro == 1
    g_half = model.brushnet.flat_g.clone()
    loss_b, norm_b = train_step(model, ns, opt, l1.to(DEV), n1.to(DEV), t1, e1.to(DEV), c1.to(DEV), gradient_accumulation_steps=2,
                                lr_scheduler=sch)
    assert norm_b is not None and opt.step_count == 1 and opt.lr == 1e-5 and opt._micro == 0
    assert float(g_half.abs().max()) > 0
    w_acc = model.brushnet.flat_w.clone()

    joint = _model("fp32").prepare_training()
    opt2 = AdamW(joint.get_trainable_modules(), lr=5e-6)
    cat = lambda a, b: torch.cat([a, b]).to(DEV)
    loss_j, norm_j = train_step(joint, ns, opt2, cat(l0, l1), cat(n0, n1), torch.cat([t0, t1]), cat(e0, e1), cat(c0, c1))
    print(f"accumulated: losses {float(loss_a):.7f} {float(loss_b):.7f} norm {float(norm_b):.6f} | joint: loss {float(loss_j):.7f} norm {float(norm_j):.6f}")
    assert abs(0.5 * (float(loss_a) + float(loss_b)) - float(loss_j)) < 1e-6 * float(loss_j)
    assert abs(float(norm_b) - float(norm_j)) < 1e-5 * float(norm_j)
    n = joint.brushnet.num_arena_floats()
    dw_acc, dw_j = w_acc[:n] - _model("fp32").prepare_training().brushnet.flat_w[:n], joint.brushnet.flat_w[:n] - _model("fp32").prepare_training().brushnet.flat_w[:n]
    # Adam's first step moves every weight by ~lr * sign(g): compare the updates, not the weights
    rel = float((dw_acc - dw_j).norm() / dw_j.norm())
    print(f"   ||update(accumulated) - update(joint)|| / ||update|| = {rel:.3e}")
    assert rel < 2e-3            # g / (|g| + eps) flips where a gradient element is ~0 (summation order differs)


# ---- round 4: configs[3] at its own width against the REFERENCE's backward pass ------------------------------------------
_FULL_SD = {}


def _full_sd(which):
    """The seeded full-size weights (tools/make_golden_r04.py::_build_train_models: UNet seed 0, BrushNet(6 ch) seed 1), drawn once."""
    if which not in _FULL_SD:
        from reflecting_reality_amd.configs import SD15_UNET, brushnet_config
        cfg = dict(SD15_UNET) if which == "unet" else dict(brushnet_config(SD15_UNET, 6))
        m = (M.UNet2DConditionModel if which == "unet" else M.BrushNetModel)(cfg, precision="fp32", device=DEV)
        _FULL_SD[which] = synth.state_dict_for(m.param_shapes(), 0 if which == "unet" else 1)
    return _FULL_SD[which]


@pytest.mark.parametrize("prec,tag,train_unet,gamma", [("fp32", "frozen", False, None), ("f16x3", "frozen", False, None),
                                                       ("bf16x1", "frozen", False, None), ("f16x3", "unet", True, 5.0),
                                                       ("fp32", "unet", True, 5.0)])
def test_baseline_config3_full_size_step_against_the_reference_backward(prec, tag, train_unet, gamma):
    """BASELINE.json configs[3]'s step at its own WIDTH against the reference's own modules under torch autograd: full-size SD1.5
    UNet + BrushNet (6 conditioning channels), batch 2 x 64 x 64 latents (512 x 512 images), loss.backward() +
    clip_grad_norm_(1.0) + one torch.optim.AdamW step (train_brushnet_mirror.py:858-888, 1407-1466), generated by
    tools/make_golden_r04.py --train-full (tests/golden/sd15_train_full.npz: loss, pre-clip gradient norm, a strided 4096-element
    sample + the full norm of 32 named BrushNet gradients — the condition stem, a zero-conv and a resnet conv per resolution
    level, samplers, norms, the time path — and ||w_1 - w_0|| of the same tensors; with --train_base_unet and --snr_gamma 5 also
    24 UNet tensors: q / k / v / out / ff at every level, proj_in, conv_in / conv_out).  Every full-size-only code path of the
    training kernels runs here: the 160 x 160 weight-gradient tiles and the pixel-split cost model, the streaming GroupNorm
    backward, the flash attention backward at 4096 tokens, the data-gradient GEMMs on the tuned inference tiles.
    fp32 and f16x3 hold the tiny fixture's bounds (2e-4 of a tensor's largest gradient, loss 1e-4, norm 2e-4); bf16x1 (the
    arithmetic of --mixed_precision=bf16) is held to the deviation the REFERENCE shows under its own bf16 mixed precision on
    this very case (tests/golden/bf16_train_full_envelope.json: ~1 % rel-L2 per tensor)."""
    import json
    G = golden("sd15_train_full.npz")
    from reflecting_reality_amd.configs import SD15_UNET, brushnet_config
    unet = M.UNet2DConditionModel(dict(SD15_UNET), precision=prec, device=DEV)
    unet.load_state_dict(_full_sd("unet"))
    bn = M.BrushNetModel(dict(brushnet_config(SD15_UNET, 6)), precision=prec, device=DEV)
    bn.load_state_dict(_full_sd("brushnet"))
    model = MirrorFusionModel(unet, bn).prepare_training(train_base_unet=train_unet)
    g = torch.Generator().manual_seed(int(G["seed"]))
    b = 2
    lat, noi = torch.randn(b, 4, 64, 64, generator=g) * 0.8, torch.randn(b, 4, 64, 64, generator=g)
    cond, ehs = torch.randn(b, 6, 64, 64, generator=g), torch.randn(b, 77, 768, generator=g)
    ts = torch.from_numpy(G["timesteps"]).long()
    ns = DDPMScheduler(**SD_SCHED)
    opt = AdamW(model.get_trainable_modules(), lr=1e-5, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    names = [k.split("/", 1)[1] for k in G.files if k.startswith(f"{tag}_grad/")]
    assert len(names) == (56 if train_unet else 32)

    allnorm = {}

    def export(mod_sd_fn, norms=False):
        out = {}
        for m in model.get_trainable_modules():
            pre = "unet." if m is model.unet else ""
            sd = mod_sd_fn(m)
            out.update({pre + k: sd[k] for k in sd if pre + k in names})
            if norms:
                allnorm.update({pre + k: float(v.double().norm()) for k, v in sd.items()})
        return out

    w0 = export(lambda m: m.state_dict())
    loss, norm = train_step(model, ns, opt, lat.to(DEV), noi.to(DEV), ts, ehs.to(DEV), cond.to(DEV), snr_gamma=gamma, max_grad_norm=1.0)
    ref_l, ref_n = float(G[f"{tag}_loss"]), float(G[f"{tag}_grad_norm"])
    print(f"[full {tag} {prec}] loss {float(loss):.7f} (reference {ref_l:.7f})  grad norm {float(norm):.6f} (reference {ref_n:.6f})")
    # NB the arena still holds this step's gradients: AdamW reads them, train_step zeroes them at the START of the next call
    grads = {k: v / model.loss_scale for k, v in export(lambda m: m.grad_state_dict(), norms=True).items()}
    w1 = export(lambda m: m.state_dict())
    env = None
    if prec == "bf16x1":
        with open(os.path.join(os.path.dirname(__file__), "golden", "bf16_train_full_envelope.json")) as f:
            env = json.load(f)
        head_ok = abs(float(loss) - ref_l) <= 2e-3 * ref_l and abs(float(norm) - ref_n) / ref_n <= max(2.0 * env["grad_norm"]["rel_dev"], 2e-3)
    else:
        # The reference's clip_grad_norm_ value is torch's fp32 norm of 619 M gradient elements (per-tensor fp32 norms, then the
        # norm of those): on this case it sits 5.6e-4 BELOW the float64 norm of the very same gradients (sqrt of the sum of the
        # squared per-parameter norms stored in the fixture: 8.436864 against 8.432162).  mf_sumsq accumulates in double, so the
        # HIP norm is held to the exact value at 2e-4 and to torch's rounded one at 1e-3.
        exact_n = float(np.sqrt((G[f"{tag}_allnorm"].astype(np.float64) ** 2).sum()))
        print(f"   total gradient norm: HIP {float(norm):.6f}, float64 norm of the reference's gradients {exact_n:.6f}, torch's fp32 clip_grad_norm_ {ref_n:.6f}")
        head_ok = abs(float(loss) - ref_l) < 1e-4 * ref_l and abs(float(norm) - exact_n) < 2e-4 * exact_n and abs(float(norm) - ref_n) < 1e-3 * ref_n
    bad, worst = ([] if head_ok else ["loss / total gradient norm"]), 0.0
    for name in names:
        ref = torch.from_numpy(G[f"{tag}_grad/{name}"]).float()
        stride = int(G[f"{tag}_gstride/{name}"])
        got_full = grads[name].float()
        got = got_full.flatten()[::stride][: ref.numel()]
        gn, ref_gn = float(got_full.double().norm()), float(G[f"{tag}_gnorm/{name}"])
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        line = f"   grad {name}: max err {err:.3e} (|ref| max {scale:.3e}) rel-L2 of the sample {rel:.2e}  ||g|| {gn:.6e} (ref {ref_gn:.6e})"
        if env is None:
            ok = err <= 2e-4 * scale + 1e-7 and abs(gn - ref_gn) <= 2e-4 * ref_gn
        else:
            e = env["grads"][name]
            worst = max(worst, rel / e["rel_l2_sample"])
            line += f"  reference under bf16: {e['rel_l2_sample']:.4f}"
            ok = rel <= 1.1 * e["rel_l2_sample"] and abs(gn - ref_gn) <= 3.0 * e["rel_l2"] * ref_gn
        print(line + ("" if ok else "   <-- FAIL"))
        if not ok:
            bad.append(name)
    if env is not None:
        print(f"   worst ratio to the reference's own bf16 deviation: {worst:.2f}")
    # EVERY parameter's gradient norm against the reference's (a wrong tensor outside the sampled list shows up here)
    ref_all = dict(zip(str(G[f"{tag}_allnorm_names"]).split("\n"), G[f"{tag}_allnorm"].tolist()))
    assert set(ref_all) == set(allnorm), sorted(set(ref_all) ^ set(allnorm))[:10]
    # (the sampled tensors above are held to 2e-4; over ALL parameters the attention q / k weights of the 32 x 32 and 16 x 16 levels
    # set the bound: their gradients are small differences of large terms in the softmax backward, fp32 itself carries ~2e-4 there
    # and the 22-bit split products four times that — measured worst case 8.1e-4 in f16x3)
    tol_n = {"fp32": 5e-4, "f16x3": 1.5e-3}[prec] if env is None else 3.0 * max(e["rel_l2"] for e in env["grads"].values())
    dev = sorted(((abs(allnorm[k] / model.loss_scale - r) / max(r, 1e-30), k) for k, r in ref_all.items()), reverse=True)
    print(f"   gradient norm of all {len(ref_all)} parameters: worst relative deviations " + ", ".join(f"{k} {d:.2e}" for d, k in dev[:6]))
    bad += [f"norm of {k}: {d:.2e}" for d, k in dev if d > tol_n and ref_all[k] > 1e-9]
    assert not bad, bad
    for name in names:                                  # one AdamW step: the movement of every named tensor
        dw, ref_dw = float((w1[name].double() - w0[name].double()).norm()), float(G[f"{tag}_dw/{name}"])
        assert abs(dw - ref_dw) < (2e-3 if env is None else 2e-2) * ref_dw, (name, dw, ref_dw)
    del model, opt, unet, bn
    torch.cuda.empty_cache()


def test_graphed_step_with_gradient_sync_is_a_chain_of_graphs_and_equals_the_eager_step(tmp_path):
    """GraphedTrainStep with a GradBuckets gradient exchange.  RCCL calls are never captured: the step is a
    chain of graphs cut where the backward pass releases a gradient bucket, the bucket's all-reduce is issued between two
    replays.  Run here with the exchange forced through RCCL on this one rank (MF_FORCE_GRAD_SYNC=1, small buckets so that the
    tiny BrushNet has several): >= 3 segments, and loss, norm and weights bit-identical to the eager synchronised step over five
    steps with changing inputs."""
    import torch.distributed as dist
    from reflecting_reality_amd import distributed as D
    from reflecting_reality_amd.training import GraphedTrainStep
    ns = DDPMScheduler(**SD_SCHED)
    os.environ["MF_FORCE_GRAD_SYNC"] = "1"
    # a file store: no port to probe, release and lose to another process (EADDRINUSE on the driver's box in round 5)
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdzv_store", rank=0, world_size=1)
    try:
        def run(graphed):
            model = _model("f16x3").prepare_training()
            opt = AdamW(model.get_trainable_modules())
            sync = D.GradBuckets(model.get_trainable_modules(), bucket_floats=64 * 1024)
            assert sync.force and sum(p["nb"] for p in sync._plan) >= 3
            step = GraphedTrainStep(model, ns, opt, warmup=2, grad_sync=sync) if graphed else None
            out = []
            for i in range(5):
                args = _skip_inputs(i)
                loss, norm = step(*args) if graphed else train_step(model, ns, opt, *args, grad_sync=sync)
                out.append((float(loss), float(norm)))
            if graphed:
                assert step.segments is not None and len(step.segments) >= 3, "the captured step must be cut at the bucket boundaries"
                sends = [a for _, a in step.segments if a is not None and a[0] is not None]
                assert len(sends) == sum(p["nb"] for p in sync._plan), "every bucket is exchanged exactly once per step"
            return model.brushnet.flat_w.clone(), out

        (wa, la), (wb, lb) = run(False), run(True)
    finally:
        dist.destroy_process_group()
        os.environ.pop("MF_FORCE_GRAD_SYNC", None)
    assert la == lb, (la, lb)
    assert torch.equal(wa, wb), "the chained-graph step with gradient sync differs from the eager one"
