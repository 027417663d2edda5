"""Device plans of the multistep schedulers (schedulers.device_plan -> mf_sched_step_dev rows), without a GPU.

Every plan is interpreted here the way the kernel runs it (include/mfhip.h, mf_sched_step_dev: registers loaded by the row's mask, the
ops in order, the masked registers stored) and compared with the scheduler's own step().  Both sides use ONE fp32 arithmetic (hip.axpby_n
and the kernel's ops are the same numpy routine here), so the final latents and the scheduler's end state must be exactly equal.  The
state starts as NaN: a plan that read a slot it had not written would show."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from reflecting_reality_amd import hip, schedulers
from reflecting_reality_amd.schedulers import PNDMScheduler, UniPCMultistepScheduler, device_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
          set_alpha_to_one=False)
SHAPE = (2, 4, 8, 8)


def _axpby(xs, cs):
    """y = c0 * x0, then y += c_k * x_k, each result rounded to fp32 (the order of mf_axpby_n and of the kernel's ops)."""
    v = np.float32(cs[0]) * xs[0]
    for c, x in zip(cs[1:], xs[1:]):
        v = (v + np.float32(c) * x).astype(np.float32)
    return v.astype(np.float32)


def _cfg(u, c, g):
    return (u + np.float32(g) * (c - u)).astype(np.float32)


@pytest.fixture
def numpy_hip(monkeypatch):
    monkeypatch.setattr(hip, "axpby_n", lambda xs, coefs, out=None: torch.from_numpy(_axpby([x.numpy() for x in xs], coefs)))


def _rows(plan):
    return [hip.SchedRow.from_buffer_copy(plan.rows[k].numpy().tobytes()) for k in range(plan.rows.shape[0])]


def _run_row(row, e, lat, state, written):
    """One mf_sched_step_dev launch in numpy.  `written`: the slots some earlier row stored (a load of any other slot is a plan error)."""
    S = row.nslots
    R = {0: e}
    for r in range(1, hip.SCHED_MAX_REGS):
        if (row.load >> r) & 1 and (r == 1 or r - 2 < S):
            if r >= 2:
                assert r - 2 in written, f"the row loads slot {r - 2}, which no earlier step wrote"
            R[r] = lat.copy() if r == 1 else state[r - 2].copy()
    for j in range(row.nops):
        op = row.ops[j]
        srcs = [op.src[k] for k in range(max(op.nterms, 1))]
        for s in srcs:
            assert s in R, f"op {j} reads register {s}, which holds nothing yet"
        R[op.dst] = R[srcs[0]].copy() if op.nterms == 0 else _axpby([R[s] for s in srcs], [op.coef[k] for k in range(op.nterms)])
    out = lat
    for r in range(1, hip.SCHED_MAX_REGS):
        if (row.store >> r) & 1:
            assert r in R and (r == 1 or r - 2 < S)
            if r == 1:
                out = R[1]
            else:
                state[r - 2] = R[r]
                written.add(r - 2)
    return out


def _same(a, b, what):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor), what
        assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                   b.view(torch.int32) if b.dtype == torch.float32 else b), what
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    else:
        assert a == b, what


def _compare(make, steps, seed=0):
    rng = np.random.default_rng(seed)
    host, dev = make(), make()
    host.set_timesteps(steps)
    dev.set_timesteps(steps)
    n = len(host.timesteps)
    x0 = rng.standard_normal(SHAPE, dtype=np.float32)
    eus = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)]
    ecs = [rng.standard_normal(SHAPE, dtype=np.float32) for _ in range(n)]
    g = 7.5
    plan = device_plan(dev)
    assert dev.__dict__.get("_step_index") is None and getattr(dev, "counter", 0) == 0, "device_plan must not step the scheduler"
    rows = _rows(plan)
    assert len(rows) == n
    lat_h = torch.from_numpy(x0.copy())
    lat_d = x0.copy()
    state = np.full((max(plan.nslots, 1),) + SHAPE, np.nan, dtype=np.float32)
    written = set()
    for k in range(n):
        e = _cfg(eus[k], ecs[k], g)
        lat_h = host.step(torch.from_numpy(e.copy()), host.timesteps[k], lat_h, return_dict=False)[0]
        lat_d = _run_row(rows[k], e, lat_d, state, written)
        assert np.array_equal(lat_h.numpy().view(np.int32), lat_d.view(np.int32)), f"step {k}: the plan's latents differ"
    plan.finish(dev, torch.from_numpy(state))
    assert set(vars(dev)) == set(vars(host))
    for key in vars(host):
        _same(getattr(dev, key), getattr(host, key), f"{type(host).__name__}.{key} after {n} steps")
    return plan, rows


def _check_rows(plan, rows):
    for k, r in enumerate(rows):
        assert 0 < r.nops <= hip.SCHED_MAX_OPS and r.nslots == plan.nslots
        assert not (r.load & 1) and not (r.store & 1), "register 0 (the guided e) is neither loaded nor stored"
        assert r.store & 2, f"row {k} does not write the latents"
        for j in range(r.nops):
            op = r.ops[j]
            assert 0 <= op.nterms <= hip.SCHED_MAX_TERMS
            assert 1 <= op.dst < hip.SCHED_MAX_REGS
            assert all(0 <= op.src[i] < hip.SCHED_MAX_REGS for i in range(max(op.nterms, 1)))
        for b in range(2, 32):
            if (r.load | r.store) >> b & 1:
                assert b - 2 < plan.nslots


UNIPC = [dict(solver_type=st, solver_order=o, prediction_type=p, lower_order_final=lof)
         for st in ("bh1", "bh2") for o in (1, 2, 3) for p in ("epsilon", "v_prediction") for lof in (True, False)]
UNIPC += [dict(solver_order=3, disable_corrector=[0, 3, 4]), dict(solver_order=2, solver_type="bh1", disable_corrector=[1])]


@pytest.mark.parametrize("steps", [10, 50])
@pytest.mark.parametrize("kw", UNIPC, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_unipc_plan_equals_the_scheduler(numpy_hip, kw, steps):
    plan, rows = _compare(lambda: UniPCMultistepScheduler(**{k: v for k, v in SD.items() if k != "set_alpha_to_one"}, **kw), steps)
    _check_rows(plan, rows)


@pytest.mark.parametrize("steps", [10, 50])
def test_unipc_from_the_pndm_config_as_the_reference_script_builds_it(numpy_hip, steps):
    """examples/brushnet/test_brushnet.py:158: UniPCMultistepScheduler.from_config(pipe.scheduler.config) over the checkpoint's PNDM."""
    base = PNDMScheduler(**SD, skip_prk_steps=True).config
    plan, rows = _compare(lambda: UniPCMultistepScheduler.from_config(base), steps)
    _check_rows(plan, rows)


@pytest.mark.parametrize("steps", [10, 50])
@pytest.mark.parametrize("skip_prk", [True, False])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_pndm_plan_equals_the_scheduler(numpy_hip, skip_prk, pred, steps):
    plan, rows = _compare(lambda: PNDMScheduler(**SD, skip_prk_steps=skip_prk, prediction_type=pred), steps)
    _check_rows(plan, rows)


def test_a_partial_plan_ends_in_the_state_of_as_many_host_steps(numpy_hip):
    """steps < len(timesteps) (SDXL's denoising_end cuts the schedule): the end state is that after exactly `steps` host steps."""
    mk = lambda: UniPCMultistepScheduler(solver_order=3, **{k: v for k, v in SD.items() if k != "set_alpha_to_one"})
    host, dev = mk(), mk()
    host.set_timesteps(12)
    dev.set_timesteps(12)
    plan = device_plan(dev, steps=7)
    assert plan.rows.shape[0] == 7
    lat = torch.zeros(SHAPE)
    for t in host.timesteps[:7]:
        lat = host.step(torch.ones(SHAPE), t, lat, return_dict=False)[0]
    plan.finish(dev, torch.zeros((plan.nslots,) + SHAPE))
    assert dev.step_index == host.step_index == 7 and dev.lower_order_nums == host.lower_order_nums and dev.this_order == host.this_order


def test_the_plan_refuses_what_it_cannot_express():
    from reflecting_reality_amd.schedulers import DDIMScheduler
    s = DDIMScheduler(**SD)
    s.set_timesteps(10)
    with pytest.raises(NotImplementedError):
        device_plan(s)
    u = UniPCMultistepScheduler()
    with pytest.raises(ValueError):
        device_plan(u)                            # set_timesteps first
    u.set_timesteps(10)
    u.last_sample = torch.zeros(SHAPE)            # a scheduler that has already stepped
    with pytest.raises(ValueError):
        device_plan(u)


def test_the_row_struct_matches_the_library():
    lib = hip.load()
    assert lib.mf_abi_version() == hip.ABI_VERSION
    assert lib.mf_sizeof_sched_row() == C.sizeof(hip.SchedRow) == 16 + hip.SCHED_MAX_OPS * (8 + 8 * hip.SCHED_MAX_TERMS)
    hdr = open(os.path.join(ROOT, "include", "mfhip.h")).read()
    for name, val in (("OPS", hip.SCHED_MAX_OPS), ("TERMS", hip.SCHED_MAX_TERMS), ("REGS", hip.SCHED_MAX_REGS)):
        assert re.search(rf"#define MF_SCHED_MAX_{name} {val}\b", hdr)


def test_the_kernel_builds_without_scratch(tmp_path):
    """mf_sched_step_dev's register file stays in VGPRs: the kernel compiles for gfx950 with 0 bytes of scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    from reflecting_reality_amd import _build
    res = subprocess.run([hipcc, *_build.HIPCC_FLAGS, "--cuda-device-only", "-c", os.path.join(_build.CSRC, "elementwise.hip"),
                          "-o", str(tmp_path / "e.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    text = res.stderr[res.stderr.index("Function Name: _ZN12_GLOBAL__N_117sched_step_kernel"):]
    text = text[:text.find("Function Name", 20) if "Function Name" in text[20:] else len(text)]
    info = {m.group(1): int(m.group(2)) for m in re.finditer(r"remark:\s+(\w+)(?: \[bytes/lane\])?: (\d+) \[", text)}
    print(f"sched_step_kernel: {info}")
    assert info["ScratchSize"] == 0 and info["VGPRs"] <= 128
