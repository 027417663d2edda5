"""The library's own random stream on the device (csrc/rng.hip) against the numpy restatement of its specification (philox_ref.py):
bits and integers exactly, normals against float64 from the same exact u and phi, moments, how draws compose (state in device memory,
shards of a global batch, the one-launch training draw), and the three users: the pipeline, the C host and the training step."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import philox_ref as PR  # noqa: E402
from reflecting_reality_amd import DDPMScheduler, hip, synth  # noqa: E402
from reflecting_reality_amd.rng import PhiloxGenerator, randn_tensor  # noqa: E402
from reflecting_reality_amd.training import (AdamW, BatchFrontEnd, GraphedTrainStep, load_state, save_state,  # noqa: E402
                                             train_step_prepared)

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1234, 2 ** 32 + 5, 2 ** 63 + 1]
OFFSETS = [0, 1, 2 ** 32 - 2]
BIG = 2 ** 20 + 3               # 262145 items (one item = one block of four outputs) on 1025 thread blocks, and a tail
# The grid is capped at 8192 x 256 threads = 2^21 items = 2^23 outputs: only a larger draw sends a thread through the grid-stride loop
# a second time.  One and a half passes (half of the threads loop, half do not), and a tail.
LOOPS = 3 * 2 ** 22 + 3
LOOPS_OFFSET = 2 ** 32 - 2 ** 21 - 5        # the block index carries into the high counter word five items into the SECOND trip


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _state(seed, offset):
    return torch.tensor([hip._s64(seed), hip._s64(offset)], dtype=torch.int64).to(DEV)


# ---- bits and integers: exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_device_bits_equal_the_oracle(seed):
    for n in (1, 3, 4, 5, 1027):
        assert np.array_equal(_u32(hip.philox_bits(n, seed, 0, DEV)), PR.bits(seed, 0, n)), n
    for offset in OFFSETS:
        assert np.array_equal(_u32(hip.philox_bits(16, seed, offset, DEV)), PR.bits(seed, offset, 16)), offset
    assert np.array_equal(_u32(hip.philox_bits(16, seed, 0, DEV)), _u32(hip.philox_bits_host(16, seed, 0)))


def test_device_bits_grid_stride_and_unaligned_output():
    got = hip.philox_bits(BIG, 1234, 2 ** 32 - 2, DEV)
    assert np.array_equal(_u32(got), PR.bits(1234, 2 ** 32 - 2, BIG))
    # an output that starts 4 bytes past a 16-byte boundary: the per-element path, nothing written outside
    buf = torch.full((1 + 1027 + 1,), 0x55555555, dtype=torch.int32, device=DEV)
    hip._launch("mf_philox_bits", buf[1:], 1027, 1234, 5, None)
    assert int(buf[0]) == 0x55555555 and int(buf[-1]) == 0x55555555
    assert np.array_equal(_u32(buf[1:-1]), PR.bits(1234, 5, 1027))


def test_draws_larger_than_the_grid_take_the_grid_stride_loop():
    """Bits, integers and normals of LOOPS elements against the oracle: every item of the second trip has the right block and address."""
    assert LOOPS > 4 * 8192 * 256 and (LOOPS + 3) // 4 < 2 * 8192 * 256
    blocks = PR.blocks(1234, LOOPS_OFFSET, PR.ceil4(LOOPS))
    want = blocks.reshape(-1)[:LOOPS]
    assert np.array_equal(_u32(hip.philox_bits(LOOPS, 1234, LOOPS_OFFSET, DEV)), want)
    got = hip.philox_randint(1000, LOOPS, 1234, LOOPS_OFFSET, DEV).cpu().numpy()
    assert np.array_equal(got, ((want.astype(np.uint64) * np.uint64(1000)) >> np.uint64(32)).astype(np.int64))
    del got, want
    z = hip.philox_normal((1, LOOPS), 1234, LOOPS_OFFSET, DEV).cpu().numpy().astype(np.float64)
    z64 = PR.normals_of(blocks, LOOPS)[None]
    assert np.all(np.abs(z - z64) <= 8 * 2.0 ** -23 * np.abs(z64))
    # three samples of a third each: sample 2 lies wholly in the second trip (per = 2^22 + 1: its rows are unaligned, too)
    per = LOOPS // 3
    z = hip.philox_normal((3, per), 7, 11, DEV)
    for s in (0, 2):
        row = hip.philox_normal((1, per), 7, 11 + s * PR.ceil4(per), DEV)
        assert torch.equal(z[s], row[0]), s


def test_empty_draws_are_empty_tensors_and_negative_counts_are_named():
    assert tuple(hip.philox_bits(0, 1, 0, DEV).shape) == (0,) and tuple(hip.philox_randint(10, 0, 1, 0, DEV).shape) == (0,)
    assert tuple(hip.philox_normal((0, 4, 8, 8), 1, 0, DEV).shape) == (0, 4, 8, 8) and tuple(hip.philox_normal((2, 0), 1, 0, DEV).shape) == (2, 0)
    g = PhiloxGenerator(5, DEV)
    assert g.randn((0, 4)).numel() == 0 and g.randint(10, 0).numel() == 0 and g.bits(0).numel() == 0 and g.offset == 0
    for call in (lambda: hip.philox_bits(-1, 1, 0, DEV), lambda: hip.philox_randint(10, -1, 1, 0, DEV)):
        with pytest.raises(hip.MfhipError, match="negative"):
            call()


@pytest.mark.parametrize("high", [1, 1000, 2 ** 31])
def test_device_integers_equal_the_oracle(high):
    for seed in SEEDS:
        for n in (1, 3, 4, 5, 1027):
            got = hip.philox_randint(high, n, seed, 0, DEV)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), PR.randint(high, seed, 0, n)), (seed, n)
        for offset in OFFSETS:
            assert np.array_equal(hip.philox_randint(high, 16, seed, offset, DEV).cpu().numpy(), PR.randint(high, seed, offset, 16))
    got = hip.philox_randint(high, BIG, 1234, 1, DEV).cpu().numpy()
    assert np.array_equal(got, PR.randint(high, 1234, 1, BIG)) and got.min() >= 0 and got.max() < high
    # a slice of a larger draw: the elements [first, first + n) only
    for first, n, total in ((3, 6, 11), (4, 4, 8), (1, 1, 2), (7, 1027, 2000)):
        got = hip.philox_randint(high, n, 1234, 9, DEV, first=first, total=total).cpu().numpy()
        assert np.array_equal(got, PR.randint(high, 1234, 9, n, first=first)), (first, n)


# ---- normals ---------------------------------------------------------------------------------------------------------------------------
NORMAL_SHAPES = [(1, 1), (1, 3), (1, 5), (3, 7), (2, 4, 8, 8), (1, BIG)]


@pytest.mark.parametrize("shape", NORMAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_normals_against_the_float64_oracle(shape):
    """|z - z64| <= 8 * 2^-23 * |z64| for every element: logf is documented to 1 ulp (halved through the square root), sqrtf 1 ulp,
    sinpif / cospif 1 ulp, half an ulp for the product — about 3 ulp in all, with a margin of two and a bit."""
    for seed, offset in ((1234, 0), (2 ** 63 + 1, 2 ** 32 - 2)):
        z = hip.philox_normal(shape, seed, offset, DEV)
        assert z.dtype == torch.float32 and tuple(z.shape) == shape
        z64 = PR.normal(shape, seed, offset)
        err = np.abs(z.cpu().numpy().astype(np.float64) - z64)
        bound = 8 * 2.0 ** -23 * np.abs(z64)
        worst = float((err / np.abs(z64)).max() / 2.0 ** -23)
        print(f"normals {shape} seed {seed}: worst relative error {worst:.3f} x 2^-23 (bound 8)")
        assert np.all(err <= bound), f"worst relative error {worst:.3f} x 2^-23"
        half = hip.philox_normal(shape, seed, offset, DEV, scale=0.5)
        assert torch.equal(half, 0.5 * z)


def test_moments_of_four_million_normals():
    """Five standard errors each: mean 1 / sqrt(n), variance sqrt(2 / n), fourth moment sqrt(96 / n), lag-1 correlation 1 / sqrt(n)."""
    n = 2 ** 22
    z = hip.philox_normal((1, n), 1234, 0, DEV).double().view(-1)
    mean, var, m4 = float(z.mean()), float(z.var(unbiased=False)), float((z ** 4).mean())
    a, b = z[:-1] - z[:-1].mean(), z[1:] - z[1:].mean()
    lag1 = float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))
    biggest = float(z.abs().max())
    print(f"mean {mean:.3e} var {var:.6f} m4 {m4:.5f} lag-1 {lag1:.3e} max |z| {biggest:.4f}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(m4 - 3) <= 5 * math.sqrt(96 / n)
    assert abs(lag1) <= 5 / math.sqrt(n)
    assert biggest <= 5.769


# ---- composition -----------------------------------------------------------------------------------------------------------------------
def test_same_seed_and_offset_same_numbers_from_host_values_or_a_device_state():
    for shape in ((3, 7), (2, 4, 8, 8)):
        a = hip.philox_normal(shape, 99, 12345, DEV)
        assert torch.equal(a, hip.philox_normal(shape, 99, 12345, DEV))
        assert torch.equal(a, hip.philox_normal(shape, 1, 1, DEV, state=_state(99, 12345)))       # the state overrides the host values
    st = _state(2 ** 63 + 1, 2 ** 32 - 2)
    assert torch.equal(hip.philox_bits(21, 0, 0, DEV, state=st), hip.philox_bits(21, 2 ** 63 + 1, 2 ** 32 - 2, DEV))
    assert torch.equal(hip.philox_randint(1000, 21, 0, 0, DEV, state=st), hip.philox_randint(1000, 21, 2 ** 63 + 1, 2 ** 32 - 2, DEV))


@pytest.mark.parametrize("tail", [(3, 5), (4, 8, 8)], ids=["per15", "per256"])
def test_shards_of_a_global_batch_concatenate_to_the_one_draw(tail):
    whole = hip.philox_normal((5,) + tail, 7, 40, DEV)
    lo = hip.philox_normal((2,) + tail, 7, 40, DEV, first_sample=0, global_batch=5)
    hi = hip.philox_normal((3,) + tail, 7, 40, DEV, first_sample=2, global_batch=5)
    assert torch.equal(torch.cat([lo, hi]), whole)
    ga, gb, gw = PhiloxGenerator(7, DEV), PhiloxGenerator(7, DEV), PhiloxGenerator(7, DEV)
    assert torch.equal(torch.cat([ga.randn((2,) + tail, 0, 5), gb.randn((3,) + tail, 2, 5)]), gw.randn((5,) + tail))
    assert ga.get_state() == gb.get_state() == gw.get_state()                                  # every rank advances by the whole draw


@pytest.mark.parametrize("present", [(False, False), (True, False), (False, True), (True, True)], ids=["image", "depth", "normals", "both"])
@pytest.mark.parametrize("shape", [(3, 4, 5, 5), (2, 3, 3, 3)], ids=["per100", "per27"])
def test_train_batch_draw_equals_the_single_entries_at_consecutive_offsets(shape, present):
    seed, offset, first, total, T = 2 ** 32 + 5, 2 ** 32 - 20, 1, 6, 1000
    b, per = shape[0], int(np.prod(shape[1:]))
    used = [True, True, *present]
    f32 = dict(dtype=torch.float32, device=DEV)
    pns = [torch.full(shape, 7.0, **f32) if u else None for u in used]
    noise, ts = torch.full(shape, 7.0, **f32), torch.full((b,), -1, dtype=torch.int64, device=DEV)
    blocks = hip.train_batch_draw(pns, noise, ts, T, seed, offset, first, total)
    o = offset
    for u, pn in zip(used, pns):
        if u:
            assert torch.equal(pn, hip.philox_normal(shape, seed, o, DEV, first_sample=first, global_batch=total))
            o += hip.philox_normal_blocks(total, per)
    assert torch.equal(noise, hip.philox_normal(shape, seed, o, DEV, first_sample=first, global_batch=total))
    o += hip.philox_normal_blocks(total, per)
    assert torch.equal(ts, hip.philox_randint(T, b, seed, o, DEV, first=first, total=total))
    assert blocks == o + hip.philox_int_blocks(total) - offset
    # the same launch reading a device state
    pns2 = [torch.empty(shape, **f32) if u else None for u in used]
    noise2, ts2 = torch.empty(shape, **f32), torch.empty(b, dtype=torch.int64, device=DEV)
    assert hip.train_batch_draw(pns2, noise2, ts2, T, 0, 0, first, total, state=_state(seed, offset)) == blocks
    assert torch.equal(noise2, noise) and torch.equal(ts2, ts) and all(x is None or torch.equal(x, y) for x, y in zip(pns2, pns))


def test_the_device_state_follows_the_host_offset():
    g = PhiloxGenerator(2 ** 63 + 1, DEV)
    g.randn((3, 7))
    g.randint(1000, 5)
    g.bits(9)
    assert g.offset == 6 + 2 + 3
    st = g.device_state()                                                                      # brought level with the host pair
    assert st.cpu().tolist() == [hip._s64(g.seed), g.offset]
    out = torch.empty(2, 4, 8, 8, device=DEV)
    hip.philox_normal(out.shape, 0, 0, DEV, state=st, out=out)
    blocks = hip.philox_normal_blocks(2, 256)
    hip.philox_advance(st, blocks)
    want = PhiloxGenerator(2 ** 63 + 1, DEV).set_state(g.get_state()).randn((2, 4, 8, 8))
    g.note_advanced(blocks, on_device=True)
    assert torch.equal(out, want)
    assert st.cpu().tolist() == [hip._s64(g.seed), g.offset] and g.device_state() is st
    g.manual_seed(5)                                                                           # the next device_state() uploads the new pair
    assert g.device_state().cpu().tolist() == [5, 0]


def test_randn_tensor_takes_philox_generators():
    a = randn_tensor((2, 4, 8, 8), PhiloxGenerator(11), DEV)
    assert a.is_cuda and torch.equal(a, hip.philox_normal((2, 4, 8, 8), 11, 0, DEV))
    b = randn_tensor((2, 4, 8, 8), [PhiloxGenerator(11), PhiloxGenerator(12)], DEV)
    assert torch.equal(b[:1], hip.philox_normal((1, 4, 8, 8), 11, 0, DEV)) and torch.equal(b[1:], hip.philox_normal((1, 4, 8, 8), 12, 0, DEV))
    with pytest.raises(ValueError):
        randn_tensor((3, 4, 8, 8), [PhiloxGenerator(11), PhiloxGenerator(12)], DEV)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pipe():
    from test_text_encoder_gpu import sd15_pipe
    return sd15_pipe("bf16", None, None), synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=32, vae_scale=2)


def _run(tiny, **kw):
    pipe, inp = tiny
    return pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
                depth=inp["depth"], num_inference_steps=3, guidance_scale=7.5, output_type="np", height=16, width=16, **kw).images


@pytest.mark.parametrize("shared", [False, True])
def test_pipeline_draws_from_a_philox_generator_in_the_documented_order(tiny_pipe, shared):
    """The conditioning noise first (2B samples, or B under cfg_shared_conditioning_sample), then the latents."""
    pipe = tiny_pipe[0]
    pipe.cfg_shared_conditioning_sample = shared
    try:
        a = _run(tiny_pipe, generator=PhiloxGenerator(7))
        b = _run(tiny_pipe, generator=PhiloxGenerator(7))
        g = PhiloxGenerator(7, DEV)
        cn = g.randn((1, 4, 8, 8)).repeat(2, 1, 1, 1) if shared else g.randn((2, 4, 8, 8))
        lat = g.randn((1, 4, 8, 8))
        c = _run(tiny_pipe, latents=lat, conditioning_noise=cn)
        used = PhiloxGenerator(7)
        _run(tiny_pipe, generator=used)
    finally:
        pipe.cfg_shared_conditioning_sample = False
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert used.get_state() == g.get_state() and not np.array_equal(a, _run(tiny_pipe, generator=PhiloxGenerator(8)))


def test_pipeline_with_a_torch_generator_is_what_it_was(tiny_pipe):
    """The conditioning noise still comes from the host's global RNG and the latents from the generator, on its device."""
    torch.manual_seed(11)
    a = _run(tiny_pipe, generator=torch.Generator(DEV).manual_seed(3))
    torch.manual_seed(11)
    cn = torch.randn(2, 4, 8, 8, dtype=torch.float32)
    lat = torch.randn((1, 4, 8, 8), generator=torch.Generator(DEV).manual_seed(3), device=DEV, dtype=torch.float32)
    assert np.array_equal(a, _run(tiny_pipe, latents=lat, conditioning_noise=cn))


def test_stochastic_scheduler_steps_draw_from_the_philox_generator(tiny_pipe):
    """eta > 0: DDIM's variance noise goes through randn_tensor, which takes the generator like the other draws."""
    g = PhiloxGenerator(7)
    a = _run(tiny_pipe, generator=g, eta=0.5)
    assert np.array_equal(a, _run(tiny_pipe, generator=PhiloxGenerator(7), eta=0.5))
    assert not np.array_equal(a, _run(tiny_pipe, generator=PhiloxGenerator(7)))
    # the conditioning noise [2, 4, 8, 8], the latents [1, 4, 8, 8], then one [1, 4, 8, 8] per step, each from where the last one ended
    one = hip.philox_normal_blocks(1, 256)
    assert g.get_state() == (7, 2 * one + one + 3 * one)
    quiet = PhiloxGenerator(7)
    _run(tiny_pipe, generator=quiet)
    assert quiet.get_state() == (7, 3 * one)                      # without eta the steps draw nothing


# ---- the C host ------------------------------------------------------------------------------------------------------------------------
def test_c_host_turns_a_seed_into_the_pipelines_image(tmp_path):
    import test_program_call_gpu as PC
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc / ROCm headers on this machine")
    exe = str(tmp_path / "inpaint_host")
    libdir = os.path.join(ROOT, "reflecting-reality_amd", "lib")
    subprocess.run([gcc, "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "examples", "c_host", "inpaint_host.c"), f"-L{libdir}", "-lmfhip", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe],
                   check=True, capture_output=True, text=True)
    pipe = PC._pipe("bf16", "ddim")
    a, b = PC._inputs(41), PC._inputs(42)
    pos, neg = PC.PROMPTS["a"]
    call_dir = str(tmp_path / "exported")
    pipe.export_call(call_dir, prompt=pos, negative_prompt=neg, image=a["image"], mask=a["mask"], depth=a["depth"], conditioning_noise=a["noise"],
                     latents=a["latents"].clone(), num_inference_steps=4, guidance_scale=7.5, height=16, width=16)
    pos, neg = PC.PROMPTS["b"]
    want = PC._as_u8(pipe(prompt=pos, negative_prompt=neg, image=PC._host_images(b["image"]), mask=PC._host_images(b["mask"]), depth=b["depth"],
                          num_inference_steps=4, guidance_scale=7.5, output_type="np", height=16, width=16, generator=PhiloxGenerator(7)).images)
    files = {}
    for name, t in (("ids", PC._ids_for("b")), ("image", b["image"]), ("mask", b["mask"]), ("depth", b["depth"])):
        files[name] = str(tmp_path / f"{name}.bin")
        t.contiguous().numpy().tofile(files[name])
    env = dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = str(tmp_path / "image_out.bin")
    args = [exe, call_dir, "--ids", files["ids"], "--image", files["image"], "--mask", files["mask"], "--depth", files["depth"], "--out", out]
    res = subprocess.run(args + ["--seed", "7"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert np.array_equal(np.fromfile(out, dtype=np.uint8).reshape(want.shape), want)
    # --seed is an alternative to the two files, not an addition
    res = subprocess.run(args + ["--seed", "7", "--latents", files["ids"]], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 2 and "--seed" in res.stderr


# ---- training --------------------------------------------------------------------------------------------------------------------------
SD_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
STEPS = 4


def _training(graphed, steps, tmp=None, resume_after=None):
    """`steps` optimisation steps from pixels with every draw from PhiloxGenerator(3): graphed (one eager warm-up, then the capture and
    replays that draw inside the graph) or eager (BatchFrontEnd + train_step_prepared).  resume_after: save there, rebuild everything,
    load, go on.  -> (trained weights, [(loss, norm)], the generator, the noise each graphed replay used)."""
    import test_train_batch_gpu as TB
    vae, ns, data = TB._vae(), DDPMScheduler(**SD_SCHED), TB._pixel_batches(steps, True)

    def fresh():
        model = TB._model("fp32", 6).prepare_training()
        opt = AdamW(model.get_trainable_modules())
        fe = BatchFrontEnd(vae, ns, depth_conditioning_mode="concat", snr_gamma=5.0)
        return model, opt, fe, GraphedTrainStep(model, ns, opt, snr_gamma=5.0, warmup=1, front_end=fe) if graphed else None

    model, opt, fe, step = fresh()
    gen, out, noises = PhiloxGenerator(3, DEV), [], []
    for i, s in enumerate(data):
        batch = TB._new_batch(s, True)
        if graphed:
            loss, norm = step.from_pixels(batch, generator=gen)
            if step._px.graph is not None:
                noises.append((step._px.draws[4].clone(), step._px.draws[5].clone()))
        else:
            loss, norm = train_step_prepared(model, ns, opt, fe(batch, generator=gen))
        out.append((float(loss), float(norm)))
        if resume_after == i + 1:
            path = save_state(str(tmp), i + 1, model, opt, generator=gen)
            model, opt, fe, step = fresh()
            gen = PhiloxGenerator(0, DEV)
            assert load_state(path, model, opt, generator=gen) == i + 1
    return TB._state(model), out, gen, noises, step


def test_front_end_draws_a_ranks_rows_and_given_tensors_still_win():
    """BatchFrontEnd.draw with a PhiloxGenerator: the samples [first_sample, first_sample + B) of the global batch, every rank advancing
    alike; a tensor the caller passes replaces its draw without shifting the others."""
    import test_train_batch_gpu as TB
    fe = BatchFrontEnd(TB._vae(), DDPMScheduler(**SD_SCHED), depth_conditioning_mode="latents")
    whole_gen = PhiloxGenerator(21, DEV)
    pns, noise, ts, _ = fe.draw({}, (3, 4, 8, 8), generator=whole_gen)
    assert [p is None for p in pns] == [False, False, False, True] and ts.dtype == torch.int64 and tuple(ts.shape) == (3,)
    assert whole_gen.offset == 4 * hip.philox_normal_blocks(3, 256) + hip.philox_int_blocks(3)
    for first, b in ((0, 1), (1, 2)):
        g = PhiloxGenerator(21, DEV)
        p2, n2, t2, _ = fe.draw({}, (b, 4, 8, 8), generator=g, first_sample=first, global_batch=3)
        assert torch.equal(n2, noise[first:first + b]) and torch.equal(t2, ts[first:first + b]) and g.get_state() == whole_gen.get_state()
        assert all(torch.equal(x, y[first:first + b]) for x, y in zip(p2[:3], pns[:3]))
    g = PhiloxGenerator(21, DEV)
    mine = torch.full((3, 4, 8, 8), 0.25)
    p3, n3, t3, _ = fe.draw({}, (3, 4, 8, 8), noise=mine, timesteps=torch.tensor([1, 2, 3]), posterior_noise=[None, mine], generator=g)
    assert torch.equal(n3.cpu(), mine) and t3.tolist() == [1, 2, 3] and torch.equal(p3[1].cpu(), mine)
    assert torch.equal(p3[0], pns[0]) and torch.equal(p3[2], pns[2]) and g.get_state() == whole_gen.get_state()
    g = PhiloxGenerator(21, DEV)                                   # everything given: nothing is drawn, the stream still moves on
    p4, n4, t4, _ = fe.draw({}, (3, 4, 8, 8), noise=mine, timesteps=torch.tensor([1, 2, 3]), posterior_noise=[mine, mine, mine], generator=g)
    assert all(torch.equal(x.cpu(), mine) for x in (*p4[:3], n4)) and t4.tolist() == [1, 2, 3] and g.get_state() == whole_gen.get_state()


@pytest.fixture(scope="module")
def graphed_run():
    return _training(True, STEPS)


def test_graphed_steps_drawing_inside_the_graph_equal_eager_draws(graphed_run):
    """Warm-up, the capture and two replays of the existing graph: losses, gradient norms and every trained weight equal the eager
    composition fed from a second generator, and both generators — and the device state — end on the same offset."""
    wa, la, ga, noises, step = graphed_run
    wb, lb, gb, _, _ = _training(False, STEPS)
    assert step._px.graph is not None and step._px.calls == STEPS and len(noises) == STEPS - 1
    assert la == lb, (la, lb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), f"{k}: the graphed steps differ from the eager ones"
    per_step = 3 * hip.philox_normal_blocks(2, 256) + hip.philox_int_blocks(2)                 # two posterior noises, the noise, the timesteps
    assert ga.get_state() == gb.get_state() == (3, STEPS * per_step)
    assert ga._state.cpu().tolist() == [3, ga.offset]


def test_replays_draw_fresh_numbers(graphed_run):
    noises = graphed_run[3]
    for (n0, t0), (n1, t1) in zip(noises, noises[1:]):
        assert not torch.equal(n0, n1) and float((n0 - n1).abs().max()) > 1.0
    assert len({tuple(t.tolist()) for _, t in noises}) == len(noises)
    assert all(0 <= int(t.min()) and int(t.max()) < 1000 for _, t in noises)


def test_a_resumed_run_continues_bit_identically(graphed_run, tmp_path):
    wa, la, ga = graphed_run[:3]
    wb, lb, gb, _, _ = _training(True, STEPS, tmp=tmp_path, resume_after=2)
    assert la == lb, (la, lb)
    assert ga.get_state() == gb.get_state()
    for k in wa:
        assert torch.equal(wa[k], wb[k]), f"{k}: the resumed run differs from the uninterrupted one"
    with pytest.raises(ValueError, match="no generator state"):
        import test_train_batch_gpu as TB
        model = TB._model("fp32", 6).prepare_training()
        load_state(save_state(str(tmp_path / "plain"), 1, model), model, generator=PhiloxGenerator(1))


def test_a_captured_step_refuses_the_other_kind_of_generator(graphed_run):
    import test_train_batch_gpu as TB
    step = graphed_run[4]
    s = TB._pixel_batches(1, True)[0]
    batch = TB._new_batch(s, True)
    with pytest.raises(ValueError, match="PhiloxGenerator"):
        step.from_pixels(batch, generator=torch.Generator(DEV).manual_seed(1))
    with pytest.raises(ValueError, match="PhiloxGenerator"):
        step.from_pixels(batch, generator=PhiloxGenerator(3, DEV))                             # another generator: another device state
    with pytest.raises(ValueError, match="given"):
        step.from_pixels(batch, noise=s["noise"], timesteps=s["ts"], posterior_noise=s["pn"])
    with pytest.raises(ValueError, match="given"):
        step.from_pixels(batch, generator=graphed_run[2], noise=s["noise"])
    # a step captured with its draws staged from outside takes no PhiloxGenerator afterwards
    vae, ns = TB._vae(), DDPMScheduler(**SD_SCHED)
    model = TB._model("fp32", 6).prepare_training()
    opt = AdamW(model.get_trainable_modules())
    old = GraphedTrainStep(model, ns, opt, warmup=1, front_end=BatchFrontEnd(vae, ns, depth_conditioning_mode="concat"))
    for _ in range(2):
        old.from_pixels(batch, noise=s["noise"], timesteps=s["ts"], posterior_noise=s["pn"])
    assert old._px.graph is not None
    with pytest.raises(ValueError, match="PhiloxGenerator"):
        old.from_pixels(batch, generator=PhiloxGenerator(3, DEV))
    old.from_pixels(batch, noise=s["noise"], timesteps=s["ts"], posterior_noise=s["pn"])      # and still takes what it was captured with
