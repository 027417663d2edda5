"""Host-side logic of LPIPS (no GPU): the geometry of the seven tapped features against torch, the first conv's packed weight, the
parameter table against torchvision's / the lpips package's key list, the sanity of the plain-torch restatement the GPU tests are measured
against (tests/lpips_ref.py), MetricsCalculator's dispatch, and the argument checks of the new C entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from reflecting_reality_amd import hip, inference, metrics
from reflecting_reality_amd.lpips import LPIPS, TAP_CHANNELS, stage_shapes
from util import GOLD

NEW = ("mf_lpips_ws_bytes", "mf_lpips_prepare", "mf_relu", "mf_maxpool3s2_ceil", "mf_lpips_layer", "mf_lpips_finish")


@pytest.fixture(scope="module")
def model():
    m = LPIPS(device="cpu")
    m.load_state_dict(R.weights(R.WEIGHT_SEED))
    return m


# ---- geometry and parameters ------------------------------------------------------------------------------------------------------------
def test_stage_shapes_are_what_torch_produces():
    """One channel is enough for the extents: the stride 2 conv without padding, then the three ceil-mode pools."""
    k = torch.zeros(1, 1, 3, 3)
    for h in range(31, 97):
        for w in range(31, 97):
            x = F.conv2d(torch.zeros(1, 1, h, w), k, stride=2)
            want = [tuple(x.shape[2:])]
            for _ in range(3):
                x = F.max_pool2d(x, 3, 2, ceil_mode=True)
                want.append(tuple(x.shape[2:]))
            assert stage_shapes(h, w) == want[:3] + [want[3]] * 4, (h, w)
    assert stage_shapes(66, 70)[0] == (32, 34) and stage_shapes(64, 64) == [(31, 31), (15, 15), (7, 7)] + [(3, 3)] * 4
    assert LPIPS.stage_shapes(512, 512)[0] == (255, 255)


@pytest.mark.parametrize("h,w", [(30, 64), (64, 30), (8, 8), (30, 30)])
def test_small_sides_are_refused(h, w, model):
    with pytest.raises(ValueError, match="at least 31 pixels"):
        stage_shapes(h, w)
    img = np.zeros((h, w, 3), np.uint8)
    with pytest.raises(ValueError):                       # (below 11 pixels to_u8_nhwc refuses first; from 11 to 30 stage_shapes does)
        metrics.lpips(img, img, model, device="cpu")
    with pytest.raises(ValueError):
        model(torch.zeros(1, h, w, 3, dtype=torch.uint8), torch.zeros(1, h, w, 3, dtype=torch.uint8))


def test_parameter_table_matches_the_published_key_list(model):
    with open(os.path.join(GOLD, "keys_lpips_squeeze.json")) as f:
        want = {k: tuple(v) for k, v in json.load(f).items()}
    got = LPIPS.param_shapes()
    assert list(got) == list(want) and dict(got) == want
    assert [got[f"lin{l}.model.1.weight"][1] for l in range(7)] == list(TAP_CHANNELS)
    sd = R.weights(R.WEIGHT_SEED)
    m = LPIPS(device="cpu").load_state_dict({**sd, "classifier.1.weight": torch.zeros(1000, 512, 1, 1), "classifier.1.bias": torch.zeros(1000)})
    assert set(m.state_dict()) == set(want)
    with pytest.raises(RuntimeError, match="unexpected"):
        LPIPS(device="cpu").load_state_dict({**sd, "features.13.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="missing"):
        LPIPS(device="cpu").load_state_dict({k: v for k, v in sd.items() if not k.startswith("lin3")})
    with pytest.raises(ValueError):
        LPIPS(precision="fp8", device="cpu")
    with pytest.raises(NotImplementedError, match="squeeze"):
        LPIPS(net_type="vgg", device="cpu")
    with pytest.raises(hip.MfhipError):
        model.train()


def test_from_pretrained_takes_files_dicts_and_a_merged_dict(tmp_path):
    from safetensors.torch import save_file
    sd = R.weights(R.WEIGHT_SEED)
    back = {k: v for k, v in sd.items() if k.startswith("features.")}
    back["classifier.1.bias"] = torch.zeros(1000)
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    torch.save(back, str(tmp_path / "squeezenet1_1.pth"))
    save_file({k: v.contiguous() for k, v in lin.items()}, str(tmp_path / "squeeze.safetensors"))
    for args in ((str(tmp_path / "squeezenet1_1.pth"), str(tmp_path / "squeeze.safetensors")), (back, lin), (sd,)):
        m = LPIPS.from_pretrained(*args, device="cpu")
        assert m.prec.name == "fp32" and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    assert LPIPS.from_pretrained(sd, precision="fp16", device="cpu").prec.name == "fp16"


def test_conv1_weight_is_packed_for_eight_channel_pixels(model):
    w = R.weights(R.WEIGHT_SEED)["features.0.weight"].numpy()            # [64, 3, 3, 3] = [n][c][ky][kx]
    want = np.zeros((64, 72), np.float32)
    for ky in range(3):
        for kx in range(3):
            for c in range(3):
                want[:, (ky * 3 + kx) * 8 + c] = w[:, c, ky, kx]
    cw = model.P["conv1"]
    assert (cw.cin, cw.cin_pad, cw.kh, cw.kw, cw.n, cw.ldw) == (3, 8, 3, 3, 64, 72)
    assert np.array_equal(cw.w.numpy(), want) and float(np.abs(want.reshape(64, 9, 8)[:, :, 3:]).max()) == 0.0
    assert torch.equal(model.P["lin2"], R.weights(R.WEIGHT_SEED)["lin2.model.1.weight"].reshape(-1))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_restatement_sanity():
    sd = R.weights(R.WEIGHT_SEED)
    assert all(float(v.min()) >= 0 for k, v in sd.items() if k.startswith("lin"))
    for h, w in ((64, 64), (66, 70)):
        pred, gt, mask = R.inputs_for(h, w)
        for region in (None, "mask", "mirror"):
            t = R.table(pred, gt, sd, torch.float64, mask, region)
            assert t.shape == (3, 7) and (t > 0).all()
            share = t / t.sum(axis=1, keepdims=True)
            print(f"{h} x {w} {region}: smallest layer share {share.min():.4f}, totals {t.sum(axis=1).round(5).tolist()}")
            assert share.min() >= 0.02, f"{h} x {w} {region}: a layer carries {share.min():.4f} of the total: change the inputs"
            assert np.array_equal(t, R.table(gt, pred, sd, torch.float64, mask, region))                     # symmetric
            for dt in (torch.float64, torch.float32, torch.bfloat16, torch.float16):
                assert float(np.abs(R.table(pred, pred, sd, dt, mask, region)).max()) == 0.0                 # identical images: exactly 0
        assert np.allclose(R.table(pred[:1], gt[:1], sd), R.table(pred, gt, sd)[:1], rtol=1e-12, atol=0)      # every pair on its own
        assert R.score(pred, gt, sd) == float(R.table(pred, gt, sd).sum(axis=1).mean())
    x = R.network_input(np.full((1, 1, 1, 3), 255, np.uint8), (-1, 1), torch.float32).reshape(-1)
    want = [np.float32(np.float32(1.0) - np.float32(s)) / np.float32(c) for s, c in zip(R.SHIFT, R.SCALE)]
    assert x.tolist() == [float(v) for v in want]
    assert float(R.network_input(np.zeros((1, 1, 1, 3), np.uint8), (0, 1), torch.float32)[0, 0, 0, 0]) == float(np.float32(0.030) / np.float32(0.458))
    with pytest.raises(ValueError, match="normalization range"):
        R.network_input(np.zeros((1, 1, 1, 3), np.uint8), (0, 255), torch.float32)


def test_finishing_rule_is_float64_on_the_host():
    rows = np.arange(1, 15, dtype=np.float32).reshape(2, 7)
    counts = np.array([a * b for a, b in stage_shapes(66, 70)], np.float64)
    got = metrics.lpips_finish(rows, 66, 70)
    assert got.dtype == np.float64 and np.array_equal(got, (rows.astype(np.float64) / counts).sum(axis=1))
    assert counts.tolist() == [32 * 34, 16 * 17, 64, 16, 16, 16, 16]


# ---- MetricsCalculator, compute_metrics, validate -----------------------------------------------------------------------------------------
def test_metrics_calculator_takes_lpips_with_a_model(model):
    calc = metrics.MetricsCalculator(["PSNR", "LPIPS", "LPIPS_mask", "LPIPS_mirror"], "cpu", lpips_model=model)
    assert calc.metrics_to_compute == ["PSNR", "LPIPS", "LPIPS_mask", "LPIPS_mirror"] and calc.lpips_model is model
    assert [calc.region_of(n) for n in calc.metrics_to_compute] == [None, None, "mask", "mirror"]
    with pytest.raises(NotImplementedError, match=r"metrics\.py:150-151"):                 # without the model: the old refusal, word for word
        metrics.MetricsCalculator(["PSNR", "LPIPS"], "cpu")
    with pytest.raises(NotImplementedError) as e:
        metrics.MetricsCalculator(["LPIPS_mask"], "cpu")
    assert str(e.value) == ("metric 'LPIPS_mask': LPIPS is not built here (the reference: metrics.py:150-151 (calculate_lpips: torchmetrics' LPIPS "
                            "network)); its network and weights are not part of this package")
    for name in ("Aesthetic_Score", "Image_Reward", "HPS_V2.1", "IoU", "LPIPS_obj", "CLIP_Similarity"):          # still refused with the model
        with pytest.raises(NotImplementedError, match=r"metrics\.py:\d+"):
            metrics.MetricsCalculator(["PSNR", name], "cpu", lpips_model=model)
        with pytest.raises(NotImplementedError):
            calc.compute_metric(name, None, {}, "a cat")
    img = np.zeros((40, 48, 3), np.uint8)
    gt = {"image": img, "masked_image": img, "mask": np.zeros((40, 48), np.uint8)}
    for name in ("LPIPS", "LPIPS_mask", "LPIPS_mirror"):
        with pytest.raises(hip.MfhipError, match="no CPU path"):                            # no CPU path behind it: host tensors are refused
            calc.compute_metric(name, img, gt, None)
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        calc.calculate_lpips(img, img)
    with pytest.raises(NotImplementedError, match="lpips_model"):
        metrics.MetricsCalculator(["PSNR"], "cpu").calculate_lpips(img, img)
    with pytest.raises(ValueError, match="needs a mask"):
        metrics.lpips_rows(img, img, model, region="mask", device="cpu")
    with pytest.raises(ValueError, match="RGB"):
        metrics.lpips_rows(np.zeros((40, 48, 4), np.uint8), np.zeros((40, 48, 4), np.uint8), model, device="cpu")
    with pytest.raises(ValueError, match="normalization range"):
        metrics.lpips(img, img, model, norm_range=[0, 255], device="cpu")


def test_compute_metrics_takes_one_lpips_not_two(model):
    img = np.zeros((40, 48, 3), np.uint8)
    with pytest.raises(ValueError, match="not both"):
        metrics.compute_metrics(img, img, lpips_fn=lambda a, b: 0.0, lpips_model=model, device="cpu")
    assert "lpips_model" in inference.validate.__kwdefaults__ and inference.validate.__kwdefaults__["lpips_model"] is None


# ---- the C entries without a device -------------------------------------------------------------------------------------------------------
def test_new_entries_exist_and_the_abi_version_stays():
    lib = hip.load()
    for name in NEW:
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert "lpips.hip" in __import__("reflecting_reality_amd._build", fromlist=["SOURCES"]).SOURCES
    assert lib.mf_abi_version() == hip.ABI_VERSION == 23          # additive entries only


def test_workspace_scales_with_the_batch():
    lib = hip.load()
    one, three = lib.mf_lpips_ws_bytes(1), lib.mf_lpips_ws_bytes(3)
    assert one >= 7 * 8 and three == 3 * one and one % 8 == 0
    assert lib.mf_lpips_ws_bytes(0) == -1 and b"batch 0" in lib.mf_last_error()
    assert lib.mf_lpips_ws_bytes(1 << 20) == -1


def test_new_entry_points_report_argument_errors():
    lib = hip.load()
    buf = (C.c_char * 8192)()
    p16 = (C.cast(buf, C.c_void_p).value + 15) // 16 * 16

    def call(fn, ok, order, **kw):
        v = {**ok, **kw}
        return fn(*[v[k] for k in order], None)

    def refuses(fn, ok, order, cases, misaligned):
        for kw, what in cases:
            assert call(fn, ok, order, **kw) == -1, kw
            assert what in lib.mf_last_error(), (kw, lib.mf_last_error())
        for kw in misaligned:
            assert call(fn, ok, order, **kw) == -3, kw
            assert b"aligned" in lib.mf_last_error()

    refuses(lib.mf_lpips_prepare, dict(pred=p16, gt=p16 + 64, mask=p16 + 128, region=0, b=1, h=33, w=35, c=3, unit=0, out=p16 + 256, dt=hip.MF_F32),
            ("pred", "gt", "mask", "region", "b", "h", "w", "c", "unit", "out", "dt"),
            ((dict(pred=None), b"null pointer"), (dict(gt=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(c=4), b"4 channels"),
             (dict(c=1), b"1 channels"), (dict(b=0), b"batch 0"), (dict(h=0), b"0 x 35"), (dict(region=3), b"region 3"),
             (dict(region=1, mask=None), b"needs a mask"), (dict(unit=2), b"unit_range 2"), (dict(dt=hip.MF_FP8), b"fp32, bf16 or fp16")),
            (dict(out=p16 + 260),))
    refuses(lib.mf_relu, dict(x=p16, dt=hip.MF_BF16, rows=4, c=16, ld=24), ("x", "dt", "rows", "c", "ld"),
            ((dict(x=None), b"null pointer"), (dict(dt=9), b"fp32, bf16 or fp16"), (dict(rows=0), b"0 rows"), (dict(c=12), b"12 channels"),
             (dict(c=0), b"0 channels"), (dict(ld=8), b"8 apart")),
            (dict(x=p16 + 8), dict(ld=20)))
    refuses(lib.mf_maxpool3s2_ceil, dict(x=p16, out=p16 + 1024, dt=hip.MF_F32, b=1, h=8, w=10, c=16), ("x", "out", "dt", "b", "h", "w", "c"),
            ((dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(dt=9), b"fp32, bf16 or fp16"), (dict(h=2), b"2 x 10"),
             (dict(w=2), b"8 x 2"), (dict(c=12), b"x 12"), (dict(b=0), b"batch 0")),
            (dict(x=p16 + 4), dict(out=p16 + 1032)))
    refuses(lib.mf_lpips_layer, dict(f=p16, dt=hip.MF_F32, w=p16 + 4096, b=1, px=255, c=64, layer=0, ws=p16 + 2048),
            ("f", "dt", "w", "b", "px", "c", "layer", "ws"),
            ((dict(f=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(dt=9), b"fp32, bf16 or fp16"),
             (dict(b=0), b"batch 0"), (dict(px=0), b"0 pixels"), (dict(px=1 << 31), b"pixels below 2^31"), (dict(c=520), b"520 channels"),
             (dict(c=60), b"60 channels"), (dict(c=0), b"0 channels"), (dict(layer=7), b"layer 7"), (dict(layer=-1), b"layer -1")),
            (dict(f=p16 + 8), dict(w=p16 + 4100), dict(ws=p16 + 2052)))
    refuses(lib.mf_lpips_finish, dict(ws=p16, b=1, out=p16 + 1024), ("ws", "b", "out"),
            ((dict(ws=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(b=0), b"batch 0")),
            (dict(ws=p16 + 4), dict(out=p16 + 1026)))
    with pytest.raises(C.ArgumentError):          # the pixel count is an int64_t, not a float
        lib.mf_lpips_layer(p16, hip.MF_F32, p16, 1, 255.0, 64, 0, p16, None)


def test_host_tensors_are_refused():
    u8 = torch.zeros(1, 33, 35, 3, dtype=torch.uint8)
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.lpips_prepare(u8, u8, None, None, False, torch.float32)
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.relu_(torch.zeros(4, 16))
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.maxpool3s2_ceil(torch.zeros(1, 8, 10, 16))
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.lpips_layer(torch.zeros(2, 3, 3, 64), torch.zeros(64), 0, torch.zeros(7 * 128 * 2))
    with pytest.raises(hip.MfhipError, match="no CPU path"):
        hip.lpips_finish(torch.zeros(7 * 128 * 2), 1)
