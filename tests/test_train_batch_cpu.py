"""The training batch on the device, the part that needs no GPU: the new entries exist in the cross-compiled library and refuse bad
arguments on the host, the Python layer refuses host tensors and malformed samples before any upload, and the reference module
(train_batch_ref.py) agrees with the ATen / numpy operations the training script and the dataset call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_header
import train_batch_ref as TR
from reflecting_reality_amd import DDPMScheduler, _build, frontend, hip

ENTRIES = ("mf_train_example_u8", "mf_masked_image_u8", "mf_fliplr", "mf_train_batch_assemble")
SD_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
P = 0x1000          # a non-null address no entry dereferences: every case below is refused on the host, before any launch


def _err(lib):
    return lib.mf_last_error().decode()


def test_new_entries_are_declared_exported_and_the_abi_version_stays():
    lib = hip.load()
    protos = abi_header.prototypes()
    for name in ENTRIES:
        assert name in protos and name in hip.SIGNATURES and hasattr(lib, name), name
    assert lib.mf_abi_version() == hip.ABI_VERSION == 23
    assert "train_batch.hip" in _build.SOURCES
    from reflecting_reality_amd import program
    for name in ENTRIES:                                   # not part of step programs
        assert name not in program.SIGNATURES and name not in program.SIGNATURES_CALL


def test_example_entries_refuse_bad_arguments_without_a_gpu():
    lib = hip.load()
    ex = lambda **kw: lib.mf_train_example_u8(*[kw.get(k, d) for k, d in (("image", P), ("mask", P), ("flips", None), ("pix", P), ("cond", P),
                                                                           ("masks", P), ("b", 2), ("h", 16), ("w", 16), ("norm", 1))], None)
    for kw, word in ((dict(image=None), "null"), (dict(mask=None), "null"), (dict(pix=None), "null"), (dict(cond=None), "null"),
                     (dict(masks=None), "null"), (dict(b=0), "positive"), (dict(h=0), "positive"), (dict(w=0), "positive"),
                     (dict(norm=2), "normalize"), (dict(pix=P + 1), "aligned")):
        assert ex(**kw) != 0 and word in _err(lib), (kw, _err(lib))
    assert lib.mf_fliplr(None, P, 5, 7, 3, None) != 0 and "null" in _err(lib)
    assert lib.mf_fliplr(P, None, 5, 7, 3, None) != 0 and "null" in _err(lib)
    assert lib.mf_fliplr(P, P, 5, 7, 3, None) != 0 and "in place" in _err(lib)
    assert lib.mf_fliplr(P, 2 * P, 0, 7, 3, None) != 0 and "positive" in _err(lib)
    assert lib.mf_fliplr(P, 2 * P, 5, 0, 3, None) != 0 and "positive" in _err(lib)
    assert lib.mf_fliplr(P, 2 * P, 5, 7, 2, None) != 0 and "channels" in _err(lib)
    assert lib.mf_masked_image_u8(None, P, P, 4, 3, 1, None) != 0 and "null" in _err(lib)
    assert lib.mf_masked_image_u8(P, P, P, 0, 3, 1, None) != 0 and "pixels" in _err(lib)
    assert lib.mf_masked_image_u8(P, P, P, 4, 5, 1, None) != 0 and "channels" in _err(lib)
    assert lib.mf_masked_image_u8(P, P, P, 4, 3, 2, None) != 0 and "invert" in _err(lib)


def _assemble(lib, **kw):
    n = kw.get("nsrc", 2)
    mom = (ctypes.c_void_p * 5)(*kw.get("moments", [P, P, None, None, None]))
    pn = (ctypes.c_void_p * 5)(*kw.get("pn", [P, P, None, None, None]))
    g = lambda k, d: kw.get(k, d)
    return lib.mf_train_batch_assemble(g("mom_arr", mom), g("pn_arr", pn), n, g("dtype", hip.MF_F32), g("ld", 16), g("c", 4), g("b", 3), g("h", 8),
                                       g("w", 8), 0.18215, g("noise", P), g("ts", P), g("sa", P), g("sb", P), g("lw", None), g("T", 1000),
                                       g("masks", P), g("depths", None), g("normals", None), g("ph", 16), g("pw", 16), g("ptype", 0),
                                       g("lat", P), g("noisy", P), g("target", P), g("cond", P), g("tsf", P), g("wout", None), None)


def test_assemble_entry_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    cases = [(dict(mom_arr=None), "null source arrays"), (dict(pn_arr=None), "null source arrays"),
             (dict(moments=[None, P, None, None, None]), "null moments"), (dict(pn=[P, None, None, None, None]), "null moments"),
             (dict(nsrc=5), "5 sources"), (dict(nsrc=1), "1 sources"), (dict(nsrc=0), "0 sources"),
             (dict(nsrc=3, moments=[P, P, P, None, None]), "source 2 needs both"),
             (dict(dtype=hip.MF_FP8), "m_dtype"), (dict(c=0), "c = 0"), (dict(c=-4), "c = -4"), (dict(ld=7), "ld 7 < 2 c"),
             (dict(b=0), "positive"), (dict(h=0), "positive"), (dict(w=0), "positive"), (dict(ph=0), "positive"), (dict(pw=0), "positive"),
             (dict(T=0), "T = 0"), (dict(T=-1), "T = -1"), (dict(ptype=2), "prediction_type 2"), (dict(ptype=-1), "prediction_type -1"),
             (dict(noise=None), "null input"), (dict(ts=None), "null input"), (dict(sa=None), "null input"), (dict(sb=None), "null input"),
             (dict(masks=None), "null input"), (dict(lat=None), "null output"), (dict(noisy=None), "null output"),
             (dict(target=None), "null output"), (dict(cond=None), "null output"), (dict(tsf=None), "null output"),
             (dict(lw=P), "go together"), (dict(wout=P), "go together"),
             (dict(nsrc=3, moments=[P, P, P, None, None], pn=[P, P, P, None, None], depths=P), "depth comes as"),
             (dict(nsrc=4, moments=[P, P, None, P, None], pn=[P, P, None, P, None], normals=P), "normals come as")]
    for kw, word in cases:
        assert _assemble(lib, **kw) != 0, kw
        assert word in _err(lib), (kw, _err(lib))


def test_host_tensors_are_refused():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.train_example_u8(u8(1, 4, 4, 3), u8(1, 4, 4))
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.masked_image_u8(u8(4, 4, 3), u8(4, 4))
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.fliplr(torch.zeros(5, 7, 3))
    z = torch.zeros
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.train_batch_assemble([z(1, 2, 2, 8), z(1, 2, 2, 8)], [z(1, 4, 2, 2)] * 2, 4, 0.18215, z(1, 4, 2, 2), z(1, dtype=torch.int64),
                                 z(10), z(10), z(1, 1, 4, 4))
    with pytest.raises(hip.MfhipError, match="2 .. 4 moment tensors"):
        hip.train_batch_assemble([z(1, 2, 2, 8)] * 5, [z(1, 4, 2, 2)] * 5, 4, 0.18215, z(1, 4, 2, 2), z(1, dtype=torch.int64), z(10), z(10),
                                 z(1, 1, 4, 4))


def test_training_example_refuses_malformed_samples_before_any_upload():
    img, mask = np.zeros((16, 16, 3), np.uint8), np.zeros((16, 16), np.uint8)
    with pytest.raises(ValueError, match="does not match"):
        frontend.training_example(dict(image=img, mask=np.zeros((16, 12), np.uint8)), resolution=16)
    with pytest.raises(ValueError, match="uint8"):
        frontend.training_example(dict(image=img.astype(np.float32), mask=mask), resolution=16)
    with pytest.raises(ValueError, match="uint8"):
        frontend.training_example(dict(image=img, mask=mask.astype(np.int32)), resolution=16)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        frontend.training_example(dict(image=np.zeros((16, 16, 4), np.uint8), mask=mask), resolution=16)
    with pytest.raises(ValueError, match="no 'depth'"):
        frontend.training_example(dict(image=img, mask=mask), resolution=16, depth=True)
    with pytest.raises(ValueError, match="one flag per sample"):
        frontend.training_example(dict(image=img[None], mask=mask[None]), resolution=16, flip=[True, False])
    with pytest.raises(ValueError, match="uint8"):
        frontend.apply_transforms_rgb(img.astype(np.float64), 16)
    with pytest.raises(ValueError, match="does not match"):
        frontend.get_masked_image(img, np.zeros((8, 8), np.uint8))


def test_front_end_refuses_unknown_modes():
    from reflecting_reality_amd.training import BatchFrontEnd
    ns = DDPMScheduler(**SD_SCHED)
    with pytest.raises(NotImplementedError, match="ip_adapter"):
        BatchFrontEnd(None, ns, normals_conditioning_mode="ip_adapter")
    with pytest.raises(ValueError, match="conditioning modes"):
        BatchFrontEnd(None, ns, depth_conditioning_mode="hint")


# ---- the reference module against the operations the script calls ---------------------------------------------------------------------
def test_reference_nearest_cat_repeat_fliplr_agree_with_aten_and_numpy():
    g = torch.Generator().manual_seed(5)
    for (hi, wi), (ho, wo) in (((16, 16), (8, 8)), ((15, 25), (6, 10)), ((512, 512), (64, 64)), ((7, 9), (7, 9)), ((5, 3), (11, 8))):
        x = torch.randn(2, 3, hi, wi, generator=g)
        assert np.array_equal(TR.nearest(x.numpy(), ho, wo), F.interpolate(x, size=(ho, wo)).numpy()), ((hi, wi), (ho, wo))
    parts = [torch.randn(3, c, 6, 10, generator=g) for c in (4, 1, 1, 3)]
    assert np.array_equal(TR.cat_channels([p.numpy() for p in parts]), torch.cat(parts, 1).numpy())
    d = torch.randn(3, 1, 15, 25, generator=g)
    assert np.array_equal(TR.repeat3(d.numpy()), d.repeat(1, 3, 1, 1).numpy())
    for shape in ((5, 7, 3), (5, 7)):
        a = torch.randn(*shape, generator=g).numpy()
        assert np.array_equal(TR.fliplr(a), np.fliplr(a))


def _sample(seed=3, h=16, w=16):
    r = np.random.RandomState(seed)
    return r.randint(0, 256, (h, w, 3)).astype(np.uint8), r.choice(np.array([0, 128, 255], np.uint8), (h, w))


def test_reference_example_is_the_datasets_arithmetic():
    img, mask = _sample()
    masked = TR.get_masked_image(img, mask)
    assert np.array_equal(masked[mask == 255], np.zeros_like(masked[mask == 255])) and np.array_equal(masked[mask != 255], img[mask != 255])
    keep = TR.get_masked_image(img, mask, invert=False)
    assert not keep[mask == 0].any() and np.array_equal(keep[mask != 0], img[mask != 0])
    for flip in (False, True):
        pix, cond, m = TR.example(img, mask, flip, 16)
        src, srcm, srck = (np.fliplr(a).copy() if flip else a for a in (img, mask, masked))
        t = lambda a: torch.from_numpy(a).float().permute(2, 0, 1) / 255.0
        assert torch.equal(pix, (t(src) - 0.5) / 0.5) and torch.equal(cond, (t(srck) - 0.5) / 0.5)
        assert torch.equal(m, (torch.from_numpy(srcm).float() / 255.0)[None])
        p0, c0, m0 = TR.example_planes(img, mask, flip)
        assert torch.equal((p0 - 0.5) / 0.5, pix) and torch.equal((c0 - 0.5) / 0.5, cond) and torch.equal(m0, m)
    # the resize path: 20 x 28 at resolution 16 -> Resize to 16 x 22 (antialiased bicubic), crop columns 3 .. 18
    img, mask = _sample(4, 20, 28)
    assert TR.resize_geometry(20, 28, 16) == ((16, 22), (0, 3)) and TR.resize_geometry(28, 20, 16) == ((22, 16), (3, 0))
    assert TR.resize_geometry(16, 16, 16) == ((16, 16), (0, 0)) and TR.resize_geometry(512, 512, 512) == ((512, 512), (0, 0))
    pix, cond, m = TR.example(img, mask, False, 16)
    whole = F.interpolate((torch.from_numpy(img).float().permute(2, 0, 1) / 255.0)[None], size=(16, 22), mode="bicubic", antialias=True,
                          align_corners=False)[0]
    assert pix.shape == (3, 16, 16) and torch.equal(pix, (whole[:, :, 3:19] - 0.5) / 0.5) and m.shape == (1, 16, 16)
    assert frontend._resize_geometry(20, 28, 16) == TR.resize_geometry(20, 28, 16)


@pytest.mark.parametrize("v_prediction", [False, True])
def test_reference_batch_agrees_with_the_scripts_fp32_arithmetic(v_prediction):
    """The float64 batch against the fp32 ATen expressions of the script (vae.py:782-791 sample, scheduling_ddpm add_noise / get_velocity,
    compute_snr weights): inside the bounds the module states for an fp32 evaluation; the data-movement outputs bit for bit."""
    g = torch.Generator().manual_seed(11)
    b, c, h, w, ld = 3, 4, 6, 10, 16
    ns = DDPMScheduler(prediction_type="v_prediction" if v_prediction else "epsilon", **SD_SCHED)
    moms = [torch.randn(b, h, w, ld, generator=g) for _ in range(3)]
    for m in moms:
        m[..., c:2 * c] *= 3.0
        m[0, 0, 0, c], m[0, 0, 1, c] = -40.0, 25.0
    pns = [torch.randn(b, c, h, w, generator=g) for _ in range(3)]
    noise, ts = torch.randn(b, c, h, w, generator=g), torch.tensor([0, 999, 500])
    masks, normals = torch.rand(b, 1, 15, 25, generator=g), torch.randn(b, 3, 15, 25, generator=g)
    ref = TR.assemble(moms, pns, c, 0.18215, noise, ts, ns.alphas_cumprod, masks, normals=normals, v_prediction=v_prediction, snr_gamma=5.0)

    def sample(m, n):
        mean, logvar = m[..., :c].permute(0, 3, 1, 2), torch.clamp(m[..., c:2 * c].permute(0, 3, 1, 2), -30.0, 20.0)
        return (mean + torch.exp(0.5 * logvar) * n) * 0.18215
    z = sample(moms[0], pns[0])
    a = ns.alphas_cumprod[ts]
    sa, sb = (a ** 0.5).reshape(-1, 1, 1, 1), ((1 - a) ** 0.5).reshape(-1, 1, 1, 1)
    assert np.all(np.abs(z.double().numpy() - ref["latents"]) <= ref["bound_latents"])
    assert np.all(np.abs((sa * z + sb * noise).double().numpy() - ref["noisy_latents"]) <= ref["bound_noisy"])
    tgt = sa * noise - sb * z if v_prediction else noise
    assert np.all(np.abs(tgt.double().numpy() - ref["target"]) <= ref["bound_target"])
    cond = torch.cat([sample(moms[1], pns[1]), F.interpolate(masks, size=(h, w)), sample(moms[2], pns[2]), F.interpolate(normals, size=(h, w))], 1)
    got = ref["conditioning_latents"]
    assert got.shape == cond.shape == (b, c + 1 + c + 3, h, w)
    assert np.array_equal(got[:, c], cond[:, c].double().numpy()) and np.array_equal(got[:, 2 * c + 1:], cond[:, 2 * c + 1:].double().numpy())
    A1, A2 = TR.posterior(moms[1], pns[1], c, 0.18215)[1], TR.posterior(moms[2], pns[2], c, 0.18215)[1]
    assert np.all(np.abs(got[:, :c] - cond[:, :c].double().numpy()) <= 2.0 ** -21 * A1)
    assert np.all(np.abs(got[:, c + 1:2 * c + 1] - cond[:, c + 1:2 * c + 1].double().numpy()) <= 2.0 ** -21 * A2)
    assert np.array_equal(ref["timesteps_f32"], ts.float().double().numpy())
    from reflecting_reality_amd.training import min_snr_weights
    wts = min_snr_weights(ns, ts, 5.0).double().numpy()
    assert np.all(np.abs(wts - ref["loss_weights"]) <= 2.0 ** -20 * np.abs(ref["loss_weights"]))


def test_schedule_tables_are_the_per_step_values_bit_for_bit():
    """BatchFrontEnd gathers from tables filled once: entry t must be what add_noise / get_velocity / training_loss compute for timestep t."""
    from reflecting_reality_amd.training import BatchFrontEnd, min_snr_weights
    for ptype in ("epsilon", "v_prediction"):
        ns = DDPMScheduler(prediction_type=ptype, **SD_SCHED)

        class _Vae:
            config = dict(latent_channels=4, scaling_factor=0.18215)
            device = "cpu"
        sa, sb, lw = BatchFrontEnd(_Vae(), ns, snr_gamma=5.0).tables("cpu")
        assert sa.dtype == sb.dtype == lw.dtype == torch.float32 and sa.numel() == sb.numel() == lw.numel() == 1000
        for ts in (torch.tensor([0, 999, 500]), torch.tensor([7, 7, 123]), torch.arange(0, 1000, 37)):
            a = ns.alphas_cumprod[ts]
            for k, t in enumerate(ts.tolist()):            # the floats add_noise hands to mf_axpby_n, through ctypes
                assert ctypes.c_float(float((a ** 0.5)[k])).value == float(sa[t]) and ctypes.c_float(float(((1 - a) ** 0.5)[k])).value == float(sb[t])
            assert torch.equal(min_snr_weights(ns, ts, 5.0).float(), lw[ts])
