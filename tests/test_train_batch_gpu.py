"""The training batch on the device (csrc/train_batch.hip, frontend.training_example, training.BatchFrontEnd / train_step_prepared /
GraphedTrainStep.from_pixels): every output against the composition of existing kernels it replaces (bit for bit) and against the float64 /
fp32 CPU reference of tests/train_batch_ref.py (inside the bounds that module states).

Measured on MI355X (largest ratio of |fp32 - float64| to the bound over every case of test_assemble_*): 0.270."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import train_batch_ref as TR  # noqa: E402
from reflecting_reality_amd import DDPMScheduler, frontend, hip, models as M, synth  # noqa: E402
from reflecting_reality_amd.configs import TINY_UNET, TINY_VAE, brushnet_config  # noqa: E402
from reflecting_reality_amd.training import (AdamW, BatchFrontEnd, EncodedBatch, GraphedTrainStep, MirrorFusionModel, compute_snr,  # noqa: E402
                                             train_step, train_step_prepared)

DEV = "cuda"
SD_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SCALING = 0.18215


def _sample(seed, h, w, b=None):
    r = np.random.RandomState(seed)
    shape = (h, w) if b is None else (b, h, w)
    return r.randint(0, 256, shape + (3,)).astype(np.uint8), r.choice(np.array([0, 128, 255], np.uint8), shape)


# ---- the example kernels --------------------------------------------------------------------------------------------------------------
def test_example_at_resolution_is_bit_equal_to_the_reference():
    """B = 2, 16 x 16 = resolution, mask values {0, 128, 255}, flips (0, 1): one launch, every output bit for bit the dataset's."""
    img, mask = _sample(1, 16, 16, b=2)
    out = frontend.training_example(dict(image=img, mask=mask), resolution=16, flip=[False, True])
    for i, flip in enumerate((False, True)):
        pix, cond, m = TR.example(img[i], mask[i], flip, 16)
        assert torch.equal(out["pixel_values"][i].cpu(), pix), f"pixel_values[{i}]"
        assert torch.equal(out["conditioning_pixel_values"][i].cpu(), cond), f"conditioning_pixel_values[{i}]"
        assert torch.equal(out["masks"][i].cpu(), m), f"masks[{i}]"
        one = frontend.training_example(dict(image=img[i], mask=mask[i]), resolution=16, flip=flip)
        assert all(torch.equal(one[k], out[k][i]) for k in out) and one["pixel_values"].shape == (3, 16, 16)
        assert torch.equal(frontend.apply_transforms_rgb(img[i], 16, flip=flip).cpu(), pix)
        assert torch.equal(frontend.apply_transforms_mask(mask[i], 16, flip=flip).cpu(), m)
    pix0, cond0 = out["pixel_values"][0].cpu(), out["conditioning_pixel_values"][0].cpu()
    grey, white = torch.from_numpy(mask[0] == 128), torch.from_numpy(mask[0] == 255)
    assert torch.equal(cond0[:, grey], pix0[:, grey]) and bool((cond0[:, white] == -1).all())       # only the value 255 blackens


@pytest.mark.parametrize("h,w", [(5, 7), (3, 1), (6, 12), (9, 18)])
def test_example_kernel_tails_and_unaligned_rows(h, w):
    """Widths that are no multiple of four (scalar tail, rows that start off a 16-byte boundary) and the dword path, flipped and not."""
    img, mask = _sample(2, h, w, b=3)
    flips = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)
    for normalize in (True, False):
        pix, cond, m = hip.train_example_u8(torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV), flips, normalize=normalize)
        for i in range(3):
            p0, c0, m0 = TR.example_planes(img[i], mask[i], bool(flips[i].item()))
            if normalize:
                p0, c0 = (p0 - 0.5) / 0.5, (c0 - 0.5) / 0.5
            assert torch.equal(pix[i].cpu(), p0) and torch.equal(cond[i].cpu(), c0) and torch.equal(m[i].cpu(), m0), (i, normalize)


def test_example_resize_path():
    """20 x 28 at resolution 16: within the existing frontend test's bound for this bicubic kernel (5e-6 on values in [-1, 1]) of torch's CPU
    antialiased interpolate, and bit-equal to the existing kernel fed the unfused planes."""
    img, mask = _sample(3, 20, 28)
    for flip in (False, True):
        out = frontend.training_example(dict(image=img, mask=mask), resolution=16, flip=flip)
        ref = TR.example(img, mask, flip, 16)
        for key, want in zip(("pixel_values", "conditioning_pixel_values", "masks"), ref):
            err = float((out[key].cpu() - want).abs().max())
            print(f"resize path {key} flip={flip}: max |err| {err:.3e}")
            assert out[key].shape == want.shape and err <= 5e-6, (key, err)
        src, srcm = (np.ascontiguousarray(np.fliplr(a)) if flip else a for a in (img, mask))
        masked = TR.get_masked_image(src, srcm)
        planes = lambda a: hip.u8_to_planes(torch.from_numpy(a).to(DEV).reshape(1, 20, 28, -1))[0]
        rs = lambda p, a, b: hip.bicubic_resize_crop(p, (16, 22), (0, 3), (16, 16), a, b, antialias=True)
        assert torch.equal(out["pixel_values"], rs(planes(src), 2.0, -1.0))
        assert torch.equal(out["conditioning_pixel_values"], rs(planes(masked), 2.0, -1.0))
        assert torch.equal(out["masks"], rs(planes(srcm), 1.0, 0.0))


def test_fliplr_and_masked_image():
    g = torch.Generator().manual_seed(9)
    for shape in ((5, 7, 3), (5, 7), (33, 130, 3), (64, 64)):
        a = torch.randn(*shape, generator=g)
        assert np.array_equal(hip.fliplr(a.to(DEV)).cpu().numpy(), np.fliplr(a.numpy())), shape
    img, mask = _sample(4, 9, 13)
    for invert in (True, False):
        got = frontend.get_masked_image(img, mask, invert=invert)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), TR.get_masked_image(img, mask, invert)), invert


def test_training_example_depth_and_normals_follow_the_flip():
    """depth / normals go through mf_fliplr and then the existing transforms: the result is what those give for np.fliplr'd inputs."""
    img, mask = _sample(5, 16, 16)
    r = np.random.RandomState(6)
    depth, normals = (r.rand(16, 16) * 4 + 0.5).astype(np.float32), r.rand(16, 16, 3).astype(np.float32)
    mask[4:9, 3:8] = 255
    for mode in ("concat", "ip_adapter"):
        out = frontend.training_example(dict(image=img, mask=mask, depth=depth, normals=normals), resolution=16, flip=True, depth=True,
                                        normals_conditioning_mode=mode)
        fd, fn, fm = (np.ascontiguousarray(np.fliplr(a)) for a in (depth, normals, mask))
        assert torch.equal(out["depths"], frontend.apply_transforms_depth(fd, mask=fm, resolution=16))
        want = frontend.mean_normal_over_mask(fn, fm) if mode == "ip_adapter" else frontend.apply_transforms_normals(fn, resolution=16)
        assert torch.equal(out["normals"], want), mode


# ---- the assemble launch ----------------------------------------------------------------------------------------------------------------
class _Vae:          # what BatchFrontEnd.assemble reads of a VAE
    config = dict(latent_channels=4, scaling_factor=SCALING)
    device = DEV


_cases: dict = {}
GEOMETRIES = {"8x8_from_16x16": ((8, 8), (16, 16)), "6x10_from_15x25": ((6, 10), (15, 25))}
RATIOS: dict = {}


def _inputs(geometry):
    """Fixed inputs of one geometry, made once and never written: B = 3, c = 4, moments with ld = 16 > 2c whose log-variances include values
    beyond the clamp (-40, 25), planes at full resolution."""
    if geometry not in _cases:
        (h, w), (ph, pw) = GEOMETRIES[geometry]
        g = torch.Generator().manual_seed(77)
        moms = []
        for _ in range(4):
            m = torch.randn(3, h, w, 16, generator=g)
            m[..., 4:8] *= 3.0
            m[0, 0, 0, 4], m[1, h - 1, w - 1, 7], m[2, 1, 2, 5] = -40.0, 25.0, 21.5
            moms.append(m)
        pns = [torch.randn(3, 4, h, w, generator=g) for _ in range(4)]
        _cases[geometry] = dict(moms=moms, pns=pns, noise=torch.randn(3, 4, h, w, generator=g), masks=torch.rand(3, 1, ph, pw, generator=g),
                                depths=torch.randn(3, 1, ph, pw, generator=g), normals=torch.randn(3, 3, ph, pw, generator=g))
    return _cases[geometry]


def _parent_weights(ns, ts, gamma, ptype):
    snr = compute_snr(ns, ts)                                                                      # training_loss, :1437-1449
    w = torch.stack([snr, gamma * torch.ones_like(snr)], dim=1).min(dim=1)[0]
    return (w / snr if ptype == "epsilon" else w / (snr + 1)).float()


@pytest.mark.parametrize("gamma", [None, 5.0])
@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("normals_mode", [None, "concat", "latents"])
@pytest.mark.parametrize("depth_mode", [None, "concat", "latents"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_assemble_equals_the_composition_it_replaces(geometry, depth_mode, normals_mode, ptype, gamma):
    """(i) every output bit-equal to hip.vae_sample + add_noise / get_velocity + hip.nearest_resize + torch.cat / hip.concat_channels +
    the compute_snr weights; (ii) within the float64 bounds of train_batch_ref.assemble.  fp32 and bf16 moments; timesteps [0, 999, 500]
    and a run with duplicates."""
    I = _inputs(geometry)
    (h, w), _ = GEOMETRIES[geometry]
    ns = DDPMScheduler(prediction_type=ptype, **SD_SCHED)
    fe = BatchFrontEnd(_Vae(), ns, depth_conditioning_mode=depth_mode, normals_conditioning_mode=normals_mode, snr_gamma=gamma)
    use = [True, True, depth_mode == "latents", normals_mode == "latents"]
    worst = 0.0
    for m_dtype in (torch.float32, torch.bfloat16):
        moms_h = [m.to(m_dtype) if u else None for m, u in zip(I["moms"], use)]
        moms = [None if m is None else m.to(DEV) for m in moms_h]
        pns = [p.to(DEV) if u else None for p, u in zip(I["pns"], use)]
        noise, masks = I["noise"].to(DEV), I["masks"].to(DEV)
        depths = I["depths"].to(DEV) if depth_mode == "concat" else None
        normals = I["normals"].to(DEV) if normals_mode == "concat" else None
        for ts in (torch.tensor([0, 999, 500]), torch.tensor([731, 12, 731])):
            got = fe.assemble(EncodedBatch(moms, pns, noise, ts.to(DEV), masks, depths, normals, None))
            # (i) the parent's composition
            z = [None if m is None else hip.vae_sample(m, p, 4, SCALING) for m, p in zip(moms, pns)]
            parts = [z[1], hip.nearest_resize(masks, h, w)]
            parts += [hip.nearest_resize(depths, h, w)] if depths is not None else ([z[2]] if z[2] is not None else [])
            parts += [hip.nearest_resize(normals, h, w)] if normals is not None else ([z[3]] if z[3] is not None else [])
            want = {"latents": z[0], "noisy_latents": ns.add_noise(z[0], noise, ts),
                    "target": noise if ptype == "epsilon" else ns.get_velocity(z[0], noise, ts),
                    "conditioning_latents": torch.cat(parts, 1), "timesteps_f32": ts.float().to(DEV)}
            if gamma is not None:
                want["loss_weights"] = _parent_weights(ns, ts, gamma, ptype).to(DEV)
            assert set(got) == set(want)
            for k in want:
                assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), f"{k} ({m_dtype}, timesteps {ts.tolist()}) is not the composition's"
            assert torch.equal(got["conditioning_latents"], hip.concat_channels(parts, 3))
            # (ii) float64
            ref = TR.assemble(moms_h, I["pns"], 4, SCALING, I["noise"], ts, ns.alphas_cumprod, I["masks"],
                              depths=I["depths"] if depths is not None else None, normals=I["normals"] if normals is not None else None,
                              v_prediction=ptype == "v_prediction", snr_gamma=gamma)
            for k, bk in (("latents", "bound_latents"), ("noisy_latents", "bound_noisy"), ("target", "bound_target")):
                err, bound = np.abs(got[k].cpu().double().numpy() - ref[k]), ref[bk]
                assert np.all(err <= bound), f"{k}: |fp32 - float64| exceeds the bound by up to {float((err - bound).max()):.3e}"
                if bound.max() > 0:
                    worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            cond, cref = got["conditioning_latents"].cpu().double().numpy(), ref["conditioning_latents"]
            at, srcs = 0, [(1, 4), ("plane", 1)] + ([("plane", 1)] if depths is not None else [(2, 4)] if use[2] else []) \
                + ([("plane", 3)] if normals is not None else [(3, 4)] if use[3] else [])
            for src, n in srcs:
                if src == "plane":
                    assert np.array_equal(cond[:, at:at + n], cref[:, at:at + n]), f"conditioning channels {at}..{at + n}"
                else:
                    bound = 2.0 ** -21 * TR.posterior(moms_h[src], I["pns"][src], 4, SCALING)[1]
                    err = np.abs(cond[:, at:at + n] - cref[:, at:at + n])
                    assert np.all(err <= bound), f"conditioning channels {at}..{at + n}"
                    worst = max(worst, float((err / bound).max()))
                at += n
            assert at == cond.shape[1] == fe.conditioning_channels()
            assert np.array_equal(got["timesteps_f32"].cpu().double().numpy(), ref["timesteps_f32"])
            if gamma is not None:      # alpha, sigma, their ratio, its square, the minimum's quotient: <= 8 roundings of half an ulp, doubled
                lw = got["loss_weights"].cpu().double().numpy()
                assert np.all(np.abs(lw - ref["loss_weights"]) <= 2.0 ** -20 * np.abs(ref["loss_weights"]))
    RATIOS[(geometry, depth_mode, normals_mode, ptype, gamma)] = worst
    print(f"largest |fp32 - float64| / bound: {worst:.3f} (over all cases so far: {max(RATIOS.values()):.3f})")


def test_assemble_clamps_device_timesteps_and_checks_host_ones():
    I = _inputs("8x8_from_16x16")
    ns = DDPMScheduler(**SD_SCHED)
    fe = BatchFrontEnd(_Vae(), ns)
    enc = lambda ts: EncodedBatch([m.to(DEV) for m in I["moms"][:2]] + [None, None], [p.to(DEV) for p in I["pns"][:2]] + [None, None],
                                  I["noise"].to(DEV), ts, I["masks"].to(DEV), None, None, None)
    inside = fe.assemble(enc(torch.tensor([0, 999, 500], device=DEV)))
    outside = fe.assemble(enc(torch.tensor([-5, 1 << 40, 500], device=DEV)))          # trusted, but clamped to the tables
    assert all(torch.equal(inside[k], outside[k]) for k in inside)
    with pytest.raises(hip.MfhipError, match="outside"):
        fe.assemble(enc(torch.tensor([0, 1000, 500])))


def test_assemble_is_capturable_no_host_dependence():
    """After one eager call the assemble step is captured with out= buffers; new timesteps, noise and planes are written into the input
    buffers and the replay gives the bits of an eager call on them.  A synchronise or a host read in the path would fail the capture."""
    I = _inputs("6x10_from_15x25")
    ns = DDPMScheduler(prediction_type="v_prediction", **SD_SCHED)
    fe = BatchFrontEnd(_Vae(), ns, depth_conditioning_mode="latents", normals_conditioning_mode="concat", snr_gamma=5.0)
    dev = lambda t: t.to(DEV).clone()
    enc = EncodedBatch([dev(m) for m in I["moms"][:3]] + [None], [dev(p) for p in I["pns"][:3]] + [None], dev(I["noise"]),
                       torch.tensor([0, 999, 500], device=DEV), dev(I["masks"]), None, dev(I["normals"]), None)
    first = fe.assemble(enc)
    bufs = {k: torch.empty_like(v) for k, v in first.items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fe.assemble(enc, out=bufs)
    graph.replay()
    assert all(torch.equal(bufs[k], first[k]) for k in first)
    g = torch.Generator().manual_seed(123)
    enc.timesteps.copy_(torch.tensor([998, 3, 3]))
    enc.noise.copy_(torch.randn(enc.noise.shape, generator=g))
    enc.masks.copy_(torch.rand(enc.masks.shape, generator=g))
    enc.normals.copy_(torch.randn(enc.normals.shape, generator=g))
    enc.moments[2].copy_(torch.randn(enc.moments[2].shape, generator=g))
    graph.replay()
    again = fe.assemble(enc)
    assert not torch.equal(again["noisy_latents"], first["noisy_latents"])
    for k in again:
        assert torch.equal(bufs[k], again[k]), f"{k}: the replay differs from an eager call on the new inputs"


# ---- end to end: two optimisation steps from uint8 images --------------------------------------------------------------------------------
def _vae():
    vae = M.AutoencoderKL(dict(TINY_VAE), precision="fp32", device=DEV)
    vae.load_state_dict(synth.state_dict_for(vae.param_shapes(), 2))
    return vae


def _model(prec, cond_channels):
    if cond_channels == 5:
        from test_training_gpu import _model as tiny_model
        return tiny_model(prec)
    unet = M.UNet2DConditionModel(dict(TINY_UNET), precision=prec, device=DEV)
    unet.load_state_dict(synth.state_dict_for(unet.param_shapes(), 0))
    bn = M.BrushNetModel(dict(brushnet_config(TINY_UNET, cond_channels)), precision=prec, device=DEV)
    bn.load_state_dict(synth.state_dict_for(bn.param_shapes(), 21))
    return MirrorFusionModel(unet, bn)


def _pixel_batches(n, depth):
    """n host samples of B = 2 decoded 16 x 16 images (the second one flipped) with the draws of each step."""
    out = []
    for i in range(n):
        img, mask = _sample(100 + i, 16, 16, b=2)
        mask[:, 3:9, 4:11] = 255
        r = np.random.RandomState(200 + i)
        g = torch.Generator().manual_seed(300 + i)
        out.append(dict(image=img, mask=mask, depth=(r.rand(2, 16, 16) * 4 + 0.5).astype(np.float32) if depth else None,
                        ehs=torch.randn(2, 77, 32, generator=g), noise=torch.randn(2, 4, 8, 8, generator=g),
                        pn=[torch.randn(2, 4, 8, 8, generator=g) for _ in range(2)], ts=torch.tensor([(37 * i + 5) % 1000, 999 - 411 * i])))
    return out


def _parent_inputs(vae, s, depth):
    """The script's lines from the reference's dataset tensors, with the kernels and ATen calls the package had before the front end."""
    flips = (False, True)
    ex = [TR.example(s["image"][i], s["mask"][i], flips[i], 16) for i in range(2)]
    pix, cpix, masks = (torch.stack([e[k] for e in ex]).to(DEV) for k in range(3))
    latents = vae.encode(pix).latent_dist.sample(noise=s["pn"][0].to(DEV)) * vae.config["scaling_factor"]
    cond = vae.encode(cpix).latent_dist.sample(noise=s["pn"][1].to(DEV)) * vae.config["scaling_factor"]
    cond = torch.cat([cond, F.interpolate(masks, size=latents.shape[-2:])], 1)
    if depth:
        fl = lambda a, i: np.ascontiguousarray(np.fliplr(a)) if flips[i] else a
        d = torch.stack([frontend.apply_transforms_depth(fl(s["depth"][i], i), mask=fl(s["mask"][i], i), resolution=16) for i in range(2)])
        cond = torch.cat([cond, F.interpolate(d, size=latents.shape[-2:])], 1)
    return latents, s["noise"].to(DEV), s["ts"], s["ehs"].to(DEV), cond


def _new_batch(s, depth):
    data = dict(image=s["image"], mask=s["mask"])
    if depth:
        data["depth"] = s["depth"]
    batch = frontend.training_example(data, resolution=16, flip=[False, True], depth=depth)
    batch["encoder_hidden_states"] = s["ehs"].to(DEV)
    return batch


def _state(model):
    return {k: v.clone() for k, v in model.brushnet.state_dict().items()}


@pytest.mark.parametrize("prec,gamma,depth", [("fp32", 5.0, False), ("bf16x1", None, True), ("fp32", None, True)])
def test_two_steps_from_pixels_equal_the_parents_composition(prec, gamma, depth):
    """Losses, gradient norms and every trained weight after step 2 are bit-equal between (TR.example tensors -> vae.encode / sample /
    * scaling_factor / F.interpolate / torch.cat -> train_step) and (training_example -> BatchFrontEnd -> train_step_prepared)."""
    vae, ns, steps = _vae(), DDPMScheduler(**SD_SCHED), _pixel_batches(2, depth)
    mode = "concat" if depth else None

    def run(new):
        model = _model(prec, 6 if depth else 5).prepare_training()
        opt = AdamW(model.get_trainable_modules())
        fe = BatchFrontEnd(vae, ns, depth_conditioning_mode=mode, snr_gamma=gamma)
        out = []
        for s in steps:
            if new:
                prepared = fe(_new_batch(s, depth), noise=s["noise"], timesteps=s["ts"], posterior_noise=s["pn"])
                loss, norm = train_step_prepared(model, ns, opt, prepared)
            else:
                loss, norm = train_step(model, ns, opt, *_parent_inputs(vae, s, depth), snr_gamma=gamma)
            out.append((float(loss), float(norm)))
        return _state(model), out

    (wa, la), (wb, lb) = run(False), run(True)
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), f"{k}: the step from pixels differs from the parent's composition"


@pytest.mark.parametrize("prec,gamma", [("fp32", 5.0), ("bf16x1", None)])
def test_graphed_from_pixels_equals_train_step_prepared_and_keeps_the_latent_path(prec, gamma):
    """GraphedTrainStep(front_end=...).from_pixels (one eager warm-up, the capture, one replay) gives train_step_prepared's bits, and
    step(latents, noise, ...) on the SAME object afterwards (warm-up, capture, replay) still gives train_step's."""
    vae, ns, steps = _vae(), DDPMScheduler(**SD_SCHED), _pixel_batches(3, True)

    def run(graphed):
        model = _model(prec, 6).prepare_training()
        opt = AdamW(model.get_trainable_modules())
        fe = BatchFrontEnd(vae, ns, depth_conditioning_mode="concat", snr_gamma=gamma)
        step = GraphedTrainStep(model, ns, opt, snr_gamma=gamma, warmup=1, front_end=fe) if graphed else None
        out = []
        for s in steps:
            kw = dict(noise=s["noise"], timesteps=s["ts"], posterior_noise=s["pn"])
            loss, norm = step.from_pixels(_new_batch(s, True), **kw) if graphed else train_step_prepared(model, ns, opt, fe(_new_batch(s, True), **kw))
            out.append((float(loss), float(norm)))
        for s in steps:
            args = _parent_inputs(vae, s, True)
            loss, norm = step(*args) if graphed else train_step(model, ns, opt, *args, snr_gamma=gamma)
            out.append((float(loss), float(norm)))
        if graphed:
            assert step._px.graph is not None and step._px.calls == 3 and step.graph is not None and step.calls == 3
        return _state(model), out

    (wa, la), (wb, lb) = run(False), run(True)
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), f"{k}: the graphed steps differ from the eager ones"


def test_front_end_draws_and_text_encoder_hook():
    """Without explicit draws the front end draws them itself (reproducibly from a device generator), and a batch with input_ids goes
    through the text encoder given at construction."""
    vae, ns = _vae(), DDPMScheduler(**SD_SCHED)
    calls = []

    def text_encoder(ids, return_dict=False):
        calls.append(ids)
        return (torch.ones(ids.shape[0], 77, 32, device=DEV) * 0.25,)
    fe = BatchFrontEnd(vae, ns, text_encoder=text_encoder)
    s = _pixel_batches(1, False)[0]
    batch = _new_batch(s, False)
    del batch["encoder_hidden_states"]
    batch["input_ids"] = torch.zeros(2, 77, dtype=torch.int64)
    a = fe(batch, generator=torch.Generator(DEV).manual_seed(1))
    b = fe(batch, generator=torch.Generator(DEV).manual_seed(1))
    assert len(calls) == 2 and a.encoder_hidden_states.shape == (2, 77, 32)
    assert a.timesteps.dtype == torch.int64 and a.timesteps.is_cuda and 0 <= int(a.timesteps.min()) and int(a.timesteps.max()) < 1000
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert (x is None and y is None) or torch.equal(x, y), f.name
    assert a.loss_weights is None and a.conditioning_latents.shape == (2, 5, 8, 8) and float(a.noise.std()) > 0.5
