"""A whole inpainting call from step programs: prompt ids, uint8 pixels, mask and depth in, a uint8 image out (program.export_encode_prompt,
pipe.export_conditioning, program.export_vae_decode(postprocess=True), pipe.export_call; mf_encode_prompt / mf_build_conditioning /
mf_decode_image; examples/c_host/inpaint_host.c).  The bar is the one tests/test_program_gpu.py sets: BITWISE equality with the Python
pipeline on inputs other than the recorded ones — the replay launches the same kernels on the same data, so no tolerance exists."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from reflecting_reality_amd import UniPCMultistepScheduler, hip, program, synth  # noqa: E402
from test_pipeline_gpu import SD_SCHED  # noqa: E402
from test_text_encoder_gpu import build_clip, sd15_pipe  # noqa: E402

try:
    import PIL.Image
except Exception:  # pragma: no cover
    PIL = None

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPTS = {"a": (["a mirror on the wall"], ["blurry"]), "b": (["two red chairs reflected in a tall glass"], ["low quality picture"])}


def _pipe(prec, sched="ddim", depth="concat"):
    te, _ = build_clip("tiny_l", prec)
    pipe = sd15_pipe(prec, te, synth.HashTokenizer(1000, 77))
    pipe.depth_conditioning_mode = depth
    if sched == "unipc":
        pipe.scheduler = UniPCMultistepScheduler(**{k: v for k, v in SD_SCHED.items() if k != "set_alpha_to_one"})
    return pipe


def _inputs(seed, batch=1, noise_batch=2):
    """uint8 pixels as a host holds them after decoding image files, the normalised depth map, the two noises"""
    g = torch.Generator().manual_seed(seed)
    image = torch.randint(0, 256, (batch, 16, 16, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros(batch, 16, 16, 3, dtype=torch.uint8)
    y, x = 2 + seed % 5, 3 + seed % 4
    mask[:, y:y + 8, x:x + 7] = 255                        # the hole
    image = image * (mask == 0)
    return dict(image=image, mask=mask, depth=torch.rand(batch, 1, 16, 16, generator=g) * 2.0 - 1.0,
                noise=torch.randn(noise_batch * batch, 4, 8, 8, generator=g), latents=torch.randn(batch, 4, 8, 8, generator=g))


def _host_images(u8):
    """What `pipe(image=...)` takes today for decoded files: PIL images (numpy float arrays of the same `/ 255.0` without PIL)"""
    if PIL is not None:
        return [PIL.Image.fromarray(a) for a in u8.numpy()]
    return u8.numpy().astype(np.float32) / 255.0


def _ids(pipe, which):
    pos, neg = PROMPTS[which]
    return pipe.tokenizer(neg + pos, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.to(DEV, torch.int32).contiguous()


# ---- 1. the ingest kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cout", [((3, 5, 7, 3), 3), ((8, 5, 7, 1), 3), ((8, 5, 7, 1), 1), ((2, 33, 37, 3), 3), ((2, 8, 8, 4), 4)])
def test_u8_to_planes_is_numpys_division_bit_for_bit(shape, cout):
    """All 256 byte values (a [2][5][7][3] tensor has 210 elements, so the batch is 3 — and 8 for the grey case), hw = 35 so that the
    tail of the four-pixel groups and the unaligned byte / scalar paths run; one shape of several blocks; one with aligned dword loads."""
    n = int(np.prod(shape))
    assert n >= 256
    vals = (np.arange(n) * 37 + 11) % 256 if n > 512 else np.arange(n) % 256
    src = vals.astype(np.uint8).reshape(shape)
    assert len(np.unique(src)) == 256
    want = (src.astype(np.float32) / 255.0).transpose(0, 3, 1, 2)
    if shape[3] == 1 and cout == 3:
        want = np.repeat(want, 3, axis=1)
    got = hip.u8_to_planes(torch.from_numpy(src).to(DEV), channels_out=cout).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_u8_to_planes_refuses_host_tensors_and_other_layouts():
    with pytest.raises(hip.MfhipError):
        hip.u8_to_planes(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(hip.MfhipError):
        hip.u8_to_planes(torch.zeros(1, 4, 4, 3, device=DEV))
    with pytest.raises(hip.MfhipError, match="channels"):
        hip.u8_to_planes(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV), channels_out=4)


# ---- 2. the prompt program --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16", "f16x3"])
def test_prompt_program_encodes_other_prompts(prec, tmp_path):
    """Exported with two prompts A ([4, 77] ids), replayed with two prompts B (other tokens, other end-of-text positions): the pipeline's
    embeddings for B in the storage dtype, with and without clip_skip; fed to the prompt-binding program: the UNet's K / V^T for B."""
    pipe = _pipe(prec)
    tok, te = pipe.tokenizer, pipe.text_encoder
    pos_a, neg_a = ["a mirror on the wall", "a cat"], ["blurry", ""]
    pos_b, neg_b = ["two red chairs reflected in a tall glass door", "sea"], ["low quality picture of nothing", "dark grain"]
    enc = lambda texts: tok(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.to(DEV, torch.int32).contiguous()
    ids_a, ids_b = enc(neg_a + pos_a), enc(neg_b + pos_b)
    assert ids_a.shape == (4, 77) and not torch.equal(ids_a.argmax(1), ids_b.argmax(1))
    act = te.prec.act
    inp = _inputs(3, batch=2)
    # the pipeline once with A (creates the K / V^T buffers), then the binding program
    pipe(prompt=pos_a, negative_prompt=neg_a, image=hip.u8_to_planes(inp["image"].to(DEV)), mask=hip.u8_to_planes(inp["mask"].to(DEV)),
         depth=inp["depth"], num_inference_steps=2, guidance_scale=7.5, latents=inp["latents"], output_type="latent", height=16, width=16,
         conditioning_noise=inp["noise"])
    pbind = str(tmp_path / "bind.mfprog")
    program.export_bind_prompt(pipe.unet, pbind)
    for clip_skip in (None, 1):
        path = str(tmp_path / f"enc{clip_skip}.mfprog")
        info = program.export_encode_prompt(te, path, ids_a, clip_skip=clip_skip)
        assert info["meta"]["entry"] == "mf_encode_prompt" and "mf_embed_tokens" in info["entries"] and "mf_act" in info["entries"]
        pe, ne = pipe.encode_prompt(pos_b, 1, True, negative_prompt=neg_b, clip_skip=clip_skip)
        want = torch.cat([ne, pe]).to(DEV, act).contiguous()
        prog = program.Program(path, DEV)
        out = torch.empty_like(want)
        hip._check(hip.load().mf_encode_prompt(prog._h, C.c_void_p(ids_b.data_ptr()), C.c_void_p(out.data_ptr()), hip._stream()), "mf_encode_prompt")
        torch.cuda.synchronize()
        assert torch.equal(out, want), f"[{prec}, clip_skip={clip_skip}] differs by {(out.float() - want.float()).abs().max()}"
        if clip_skip is None:
            # K / V^T: the pipeline's own binding of B, then the program pair on memory of its own
            assert pipe.unet.bind_prompt(torch.cat([ne, pe]).to(DEV))
            torch.cuda.synchronize()
            kv = {b: (v[0].clone(), v[1].clone(), v[0].data_ptr(), v[1].data_ptr()) for b, v in pipe.unet._cross_kv.items()}
            bind = program.Program(pbind, DEV)
            bind.write("prompt_embeds", out)
            bind.run()
            torch.cuda.synchronize()
            assert kv
            for b, (k, vt, pk, pvt) in kv.items():
                for t, ptr in ((k, pk), (vt, pvt)):
                    got = bind.buffer(f"const.{ptr:x}")[:t.numel() * t.element_size()].view(t.dtype).view(t.shape)
                    assert torch.equal(got, t), f"{b}: K / V^T written by the programs differ from the pipeline's"
            bind.close()
        prog.close()


# ---- 3. the conditioning program --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("depth", [None, "concat"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conditioning_program_builds_cond_from_pixels(prec, depth, shared, tmp_path):
    pipe = _pipe(prec, depth=depth)
    a, b = _inputs(11, noise_batch=1 if shared else 2), _inputs(12, noise_batch=1 if shared else 2)
    path = str(tmp_path / "cond.mfprog")
    info = pipe.export_conditioning(path, image=a["image"], mask=a["mask"], depth=a["depth"] if depth else None, conditioning_noise=a["noise"])
    meta = info["meta"]
    assert meta["entry"] == "mf_build_conditioning" and meta["cond_noise_batch"] == (1 if shared else 2) and meta["brushnet_once"] == shared
    assert "mf_u8_to_planes" in info["entries"] and "mf_mask_keep" in info["entries"] and "mf_vae_sample" in info["entries"]
    noise_full = b["noise"].repeat(2, 1, 1, 1) if shared else b["noise"]
    dep = b["depth"] if depth else None
    want = pipe.build_conditioning(hip.u8_to_planes(b["image"].to(DEV)), hip.u8_to_planes(b["mask"].to(DEV)), dep.to(DEV) if depth else None,
                                   16, 16, 1, 1, True, noise_full)
    assert pipe._brushnet_shareable(want, 1, True) == shared
    want_pil = pipe.build_conditioning(_host_images(b["image"]), _host_images(b["mask"]), dep, 16, 16, 1, 1, True, noise_full)
    assert torch.equal(want, want_pil), "the uint8 ingest and the PIL path of preprocess disagree"
    assert want.shape == (2, 6 if depth else 5, 8, 8)
    prog = program.Program(path, DEV)
    cond = torch.empty_like(want)
    dev = {k: b[k].to(DEV).contiguous() for k in ("image", "mask", "depth", "noise")}
    hip._check(hip.load().mf_build_conditioning(prog._h, C.c_void_p(dev["image"].data_ptr()), C.c_void_p(dev["mask"].data_ptr()),
                                                C.c_void_p(dev["depth"].data_ptr()) if depth else None, C.c_void_p(dev["noise"].data_ptr()),
                                                C.c_void_p(cond.data_ptr()), hip._stream()), "mf_build_conditioning")
    torch.cuda.synchronize()
    assert torch.equal(cond, want), f"cond differs by {(cond - want).abs().max()}"
    # the other noise form than the exported one is refused with a message
    other = torch.zeros(2 if shared else 1, 4, 8, 8)
    with pytest.raises(program.ProgramError, match="exported for"):
        prog.write("cond_noise", other)
    if not depth:
        rc = hip.load().mf_build_conditioning(prog._h, None, None, C.c_void_p(dev["depth"].data_ptr()), None, None, hip._stream())
        assert rc != 0 and b"depth" in hip.load().mf_last_error()
    prog.close()


# ---- 4. decode + postprocess ------------------------------------------------------------------------------------------------------
def _call(pipe, which, inp, steps, out, **kw):
    pos, neg = PROMPTS[which]
    return pipe(prompt=pos, negative_prompt=neg, image=_host_images(inp["image"]), mask=_host_images(inp["mask"]), depth=inp["depth"],
                num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"].clone(), output_type=out, height=16, width=16,
                conditioning_noise=inp["noise"], **kw).images


def _as_u8(np_image):
    return (np_image * 255).round().astype("uint8")          # VaeImageProcessor.postprocess's own rounding (numpy: half to even, as rintf)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_decode_program_with_postprocess(prec, tmp_path):
    pipe = _pipe(prec)
    a, b = _inputs(21), _inputs(22)
    lat_a = _call(pipe, "a", a, 3, "latent")
    path = str(tmp_path / "dec.mfprog")
    info = program.export_vae_decode(pipe.vae, path, lat_a, postprocess=True)
    assert info["meta"]["entry"] == "mf_decode_image" and "mf_postprocess" in info["entries"] and "mf_axpby_n" in info["entries"]
    lat_b = _call(pipe, "b", b, 3, "latent").to(DEV).float().contiguous()
    want = _as_u8(_call(pipe, "b", b, 3, "np"))
    prog = program.Program(path, DEV)
    out = torch.empty(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    hip._check(hip.load().mf_decode_image(prog._h, C.c_void_p(lat_b.data_ptr()), C.c_void_p(out.data_ptr()), hip._stream()), "mf_decode_image")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    prog.close()


def test_plain_vae_decode_export_is_unchanged(tmp_path):
    """Without the new argument export_vae_decode writes the program it wrote before: "z" in, fp32 "image" out, the same calls."""
    pipe = _pipe("bf16")
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    info = program.export_vae_decode(pipe.vae, str(tmp_path / "d.mfprog"), z)
    assert info["meta"]["entry"] == "mf_vae_decode" and "mf_postprocess" not in info["entries"] and "mf_axpby_n" not in info["entries"]
    prog = program.Program(str(tmp_path / "d.mfprog"), DEV)
    assert set(n for n in prog.names if "." not in n) == {"z", "image"}
    prog.close()


# ---- 5. the whole call from Python, programs alone -------------------------------------------------------------------------------
def _drive(directory, ids, inp, sigma=1.0):
    """encode -> bind -> conditioning -> N steps -> decode with program.Program alone; (uint8 image, final latents)"""
    with open(os.path.join(directory, "manifest.json")) as f:
        man = json.load(f)
    p = lambda k: os.path.join(directory, man["files"][k])
    step = program.Program(p("step"), DEV)
    bind = program.Program(p("bind_prompt"), DEV, share=step)
    enc = program.Program(p("encode_prompt"), DEV, share=bind, only=("prompt_embeds",))
    cond = program.Program(p("conditioning"), DEV, share=step, only=("cond",))
    dec = program.Program(p("decode"), DEV, share=step, only=("latents",))
    enc.write("input_ids", ids)
    enc.run()
    bind.run()
    cond.write("image_u8", inp["image"]); cond.write("mask_u8", inp["mask"]); cond.write("cond_noise", inp["noise"])
    if man["depth"]:
        cond.write("depth", inp["depth"])
    cond.run()
    step.write("latents", inp["latents"] * sigma)
    tables = [n for n in step.names if n.startswith("table.")]
    for i in range(man["steps"]):
        for n in tables:
            row = step.buffer(n[6:])
            row.copy_(step.buffer(n).view(man["steps"], -1)[i])
        step.run()
    dec.run()
    torch.cuda.synchronize()
    out = (dec.buffer("image_u8").view(1, 16, 16, 3).cpu().numpy().copy(), step.buffer("latents", torch.float32).view(1, 4, 8, 8).cpu().clone())
    for q in (dec, cond, enc, bind, step):
        q.close()
    return out


@pytest.mark.parametrize("sched,steps", [("ddim", 4), ("unipc", 5)])
@pytest.mark.parametrize("prec", ["bf16", "f16x3"])
def test_whole_call_from_programs(prec, sched, steps, tmp_path):
    pipe = _pipe(prec, sched)
    a, b = _inputs(31), _inputs(32)
    pos, neg = PROMPTS["a"]
    info = pipe.export_call(str(tmp_path), prompt=pos, negative_prompt=neg, image=a["image"], mask=a["mask"], depth=a["depth"],
                            conditioning_noise=a["noise"], latents=a["latents"].clone(), num_inference_steps=steps, guidance_scale=7.5,
                            height=16, width=16)
    man = info["manifest"]
    assert man["steps"] == steps and man["abi_version"] == hip.ABI_VERSION and man["cond_noise_batch"] == 2 and not man["brushnet_once"]
    assert sorted(os.listdir(tmp_path)) == sorted(list(man["files"].values()) + ["manifest.json", "manifest.txt"])
    want_lat = _call(pipe, "b", b, steps, "latent").float().cpu()
    want_img = _as_u8(_call(pipe, "b", b, steps, "np"))
    assert not torch.equal(want_lat, info["result"].images.float().cpu())
    del pipe
    img, lat = _drive(str(tmp_path), _ids_for("b"), b, sigma=float(man["init_noise_sigma"]))
    assert torch.equal(lat, want_lat), f"[{prec} {sched}] final latents differ by {(lat - want_lat).abs().max()}"
    assert np.array_equal(img, want_img)


def _ids_for(which):
    pos, neg = PROMPTS[which]
    return synth.HashTokenizer(1000, 77)(neg + pos, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.to(torch.int32)


# ---- 6. the C host ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exported_call(tmp_path_factory):
    """One export (bf16, UniPC, 5 steps) and the pipeline's answer for inputs B, shared by the C-host cases; the host is built with gcc as
    tests/test_program_gpu.py builds denoise_host.c."""
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no gcc / ROCm headers on this machine")
    d = tmp_path_factory.mktemp("call")
    exe = str(d / "inpaint_host")
    libdir = os.path.join(ROOT, "reflecting-reality_amd", "lib")
    subprocess.run([gcc, "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "examples", "c_host", "inpaint_host.c"), f"-L{libdir}", "-lmfhip", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe],
                   check=True, capture_output=True, text=True)
    pipe = _pipe("bf16", "unipc")
    a, b = _inputs(41), _inputs(42)
    pos, neg = PROMPTS["a"]
    call_dir = d / "exported"
    pipe.export_call(str(call_dir), prompt=pos, negative_prompt=neg, image=a["image"], mask=a["mask"], depth=a["depth"], conditioning_noise=a["noise"],
                     latents=a["latents"].clone(), num_inference_steps=5, guidance_scale=7.5, height=16, width=16)
    want_img = _as_u8(_call(pipe, "b", b, 5, "np"))
    want_lat = _call(pipe, "b", b, 5, "latent").float().cpu()
    files = {}
    for name, t in (("ids", _ids_for("b")), ("image", b["image"]), ("mask", b["mask"]), ("depth", b["depth"]), ("noise", b["noise"]),
                    ("latents", b["latents"])):
        files[name] = str(d / f"{name}.bin")
        t.contiguous().numpy().tofile(files[name])
    env = dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    return dict(exe=exe, dir=str(call_dir), files=files, env=env, image=want_img, latents=want_lat, tmp=d)


def _host_args(ex, out, **over):
    f = dict(ex["files"], **over)
    return [ex["exe"], over.get("dir", ex["dir"]), "--ids", f["ids"], "--image", f["image"], "--mask", f["mask"], "--depth", f["depth"], "--noise", f["noise"],
            "--latents", f["latents"], "--out", out]


@pytest.mark.parametrize("graph", [False, True])
def test_c_host_inpaints_without_python(graph, exported_call, tmp_path):
    ex = exported_call
    out, lat_out = str(tmp_path / "image_out.bin"), str(tmp_path / "latents_out.bin")
    res = subprocess.run(_host_args(ex, out) + ["--latents-out", lat_out] + (["--graph"] if graph else []), capture_output=True, text=True,
                         timeout=600, env=ex["env"])
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    lat = torch.from_numpy(np.fromfile(lat_out, dtype=np.float32)).view(ex["latents"].shape)
    assert torch.equal(lat, ex["latents"]), f"the C host's latents differ from the pipeline's by {(lat - ex['latents']).abs().max()}"
    assert np.array_equal(np.fromfile(out, dtype=np.uint8).reshape(ex["image"].shape), ex["image"])


def test_c_host_checks_its_inputs_before_the_device(exported_call, tmp_path):
    """A wrong-sized ids.bin and a manifest that names a missing file end the host with a message while it is still reading files:
    nothing was allocated or launched, and no output exists."""
    ex = exported_call
    out = str(tmp_path / "image_out.bin")
    short = str(tmp_path / "ids_short.bin")
    np.fromfile(ex["files"]["ids"], dtype=np.int32)[:-7].tofile(short)
    res = subprocess.run(_host_args(ex, out, ids=short), capture_output=True, text=True, timeout=120, env=ex["env"])
    assert res.returncode != 0 and "input_ids" in res.stderr and not os.path.exists(out), res.stderr
    broken = tmp_path / "broken"
    shutil.copytree(ex["dir"], broken)
    text = (broken / "manifest.txt").read_text().replace("files.decode decode.mfprog", "files.decode nowhere.mfprog")
    (broken / "manifest.txt").write_text(text)
    res = subprocess.run(_host_args(ex, out, dir=str(broken)), capture_output=True, text=True, timeout=120, env=ex["env"])
    assert res.returncode != 0 and "nowhere.mfprog" in res.stderr and not os.path.exists(out), res.stderr


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_each_others_programs(tmp_path):
    pipe = _pipe("bf16")
    a = _inputs(51)
    ids = _ids(pipe, "a")
    penc, pstep = str(tmp_path / "enc.mfprog"), str(tmp_path / "step.mfprog")
    program.export_encode_prompt(pipe.text_encoder, penc, ids)
    pos, neg = PROMPTS["a"]
    pipe.export_denoise_step(pstep, prompt=pos, negative_prompt=neg, image=hip.u8_to_planes(a["image"].to(DEV)), mask=hip.u8_to_planes(a["mask"].to(DEV)),
                             depth=a["depth"], num_inference_steps=3, guidance_scale=7.5, latents=a["latents"].clone(), height=16, width=16,
                             conditioning_noise=a["noise"])
    lib = hip.load()
    enc, step = program.Program(penc, DEV), program.Program(pstep, DEV)
    buf = torch.zeros(4096, device=DEV)
    assert lib.mf_encode_prompt(step._h, None, None, hip._stream()) != 0 and b"mf_encode_prompt" in lib.mf_last_error()
    assert lib.mf_decode_image(step._h, None, None, hip._stream()) != 0 and b"not exported for this entry" in lib.mf_last_error()
    assert lib.mf_build_conditioning(enc._h, None, None, None, None, None, hip._stream()) != 0 and b"mf_build_conditioning" in lib.mf_last_error()
    assert lib.mf_denoise_step_fused(enc._h, C.c_void_p(buf.data_ptr()), None, None, None, hip._stream()) != 0 and b"latents" in lib.mf_last_error()
    enc.close(); step.close()


def test_exports_refuse_what_a_program_cannot_hold(tmp_path):
    from test_ip_adapter_gpu import checkpoint
    a = _inputs(61)
    # a mode whose recording meets a torch kernel: 'latents' depth conditioning repeats the depth map to three channels (aten::repeat)
    pipe = _pipe("bf16", depth="latents")
    path = tmp_path / "cond.mfprog"
    with pytest.raises(program.ProgramError, match="aten::"):
        pipe.export_conditioning(str(path), image=a["image"], mask=a["mask"], depth=a["depth"], conditioning_noise=a["noise"])
    assert not path.exists() and hip._RECORDER is None
    # several images per prompt: repeat_interleave (an expanded source copied row over row)
    pipe = _pipe("bf16")
    with pytest.raises(program.ProgramError, match="broadcasting torch copy"):
        pipe.export_conditioning(str(path), image=a["image"], mask=a["mask"], depth=a["depth"], conditioning_noise=a["noise"].repeat(2, 1, 1, 1),
                                 num_images_per_prompt=2)
    assert not path.exists() and hip._RECORDER is None
    with pytest.raises(program.ProgramError, match="uint8 pixels"):
        pipe.export_conditioning(str(path), image=torch.rand(1, 3, 16, 16), mask=a["mask"], depth=a["depth"], conditioning_noise=a["noise"])
    # IP-Adapter processors on the UNet: the existing refusal, before anything is written
    pipe.unet.load_ip_adapter(checkpoint())
    pos, neg = PROMPTS["a"]
    with pytest.raises(program.ProgramError, match="has no replay thunk"):
        pipe.export_call(str(tmp_path / "call"), prompt=pos, negative_prompt=neg, image=a["image"], mask=a["mask"], depth=a["depth"],
                         conditioning_noise=a["noise"], latents=a["latents"].clone(), num_inference_steps=3, height=16, width=16)
    assert not (tmp_path / "call").exists()
