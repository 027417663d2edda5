"""Export the denoise step of BASELINE configs[1] (batch 4 x 512 x 512, 50-step DDIM, CFG 7.5) as a step program, run the whole
loop from a C host with no Python in the process (examples/c_host/denoise_host.c), and compare its latents with the pipeline's.
usage: python tools/export_step.py [--precision bf16] [--steps 50] [--out /tmp/step.mfprog]
       python tools/export_step.py --call [--precision bf16] [--steps 50] [--out /tmp/call_dir] [--repeats 3]
--call: export the WHOLE call (pipe.export_call: prompt encoding, prompt binding, conditioning, step, decode) and run it from
examples/c_host/inpaint_host.c; its uint8 image is compared with the pipeline's, and the host's time from the first upload to the image
on the host is printed next to the wall time of `pipe(...)` on the same inputs, the two alternating."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from reflecting_reality_amd import hip, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="bf16")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=None)
ap.add_argument("--call", action="store_true")
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
a.out = a.out or ("/tmp/call_dir" if a.call else "/tmp/step.mfprog")
dev = torch.device("cuda", 0)
hip.load()
pipe, _ = bench.build_pipeline(a.precision, dev)


def whole_call():
    import re
    import shutil
    from reflecting_reality_amd.configs import CLIP_L_TEXT
    from reflecting_reality_amd.text_encoder import CLIPTextModel
    te = CLIPTextModel(dict(CLIP_L_TEXT), precision=a.precision, device=dev)
    te.load_state_dict(synth.state_dict_for(te.param_shapes(), 3))
    pipe.text_encoder, pipe.tokenizer = te, synth.HashTokenizer(int(CLIP_L_TEXT["vocab_size"]), 77)
    g = torch.Generator().manual_seed(1234)
    image = torch.randint(0, 256, (4, 512, 512, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros(4, 512, 512, 3, dtype=torch.uint8)
    mask[:, 128:384, 128:384] = 255
    image = image * (mask == 0)
    depth = torch.rand(4, 1, 512, 512, generator=g) * 2.0 - 1.0
    noise, latents = torch.randn(8, 4, 64, 64, generator=g), torch.randn(4, 4, 64, 64, generator=g)
    prompts = [f"a mirror reflecting scene number {i} of a quiet room" for i in range(4)]
    neg = ["blurry, low quality"] * 4
    kw = dict(prompt=prompts, negative_prompt=neg, depth=depth, num_inference_steps=a.steps, guidance_scale=7.5, latents=latents,
              brushnet_conditioning_scale=1.0, height=512, width=512, conditioning_noise=noise)
    t0 = time.time()
    info = pipe.export_call(a.out, image=image, mask=mask, **kw)
    size = sum(os.path.getsize(os.path.join(a.out, f)) for f in os.listdir(a.out))
    print(f"exported in {time.time() - t0:.1f} s: {size / 1e9:.3f} GB in {sorted(os.listdir(a.out))}; "
          + ", ".join(f"{k}: {v['calls']} calls" for k, v in info["programs"].items()))
    exe, libdir = "/tmp/inpaint_host", os.path.join(ROOT, "reflecting-reality_amd", "lib")
    subprocess.run(["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "examples", "c_host", "inpaint_host.c"), f"-L{libdir}", "-lmfhip", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
    ids = pipe.tokenizer(neg + prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.to(torch.int32)
    files = {}
    for name, t in (("ids", ids), ("image", image), ("mask", mask), ("depth", depth), ("noise", noise), ("latents", latents)):
        files[name] = f"/tmp/call_{name}.bin"
        t.contiguous().numpy().tofile(files[name])
    planes = lambda u8: hip.u8_to_planes(u8.to(dev))
    env = dict(os.environ, LD_LIBRARY_PATH=f"{libdir}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    cmd = [exe, a.out] + [x for k in files for x in (f"--{k}", files[k])] + ["--out", "/tmp/call_image_out.bin"]
    py_ms, c_ms, want = [], [], None
    for r in range(a.repeats + 1):                  # (the first pair warms both sides and is not reported)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = pipe(image=planes(image), mask=planes(mask), output_type="np", **kw).images
        t1 = time.perf_counter()
        want = (img * 255).round().astype("uint8")
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
        if out.returncode != 0:
            print(out.stdout + out.stderr)
            return
        if r:
            py_ms.append((t1 - t0) * 1e3)
            c_ms.append(float(re.search(r"([0-9.]+) ms from the first upload", out.stdout).group(1)))
    got = np.fromfile("/tmp/call_image_out.bin", dtype=np.uint8).reshape(want.shape)
    print("C host image == pipeline image (bitwise):", bool(np.array_equal(got, want)), "differing bytes:", int((got != want).sum()))
    print(f"pipe(...) wall time, ms: {[round(x, 1) for x in py_ms]}; C host, first upload -> image on the host, ms: {[round(x, 1) for x in c_ms]}")
    # stage by stage from this process: each program against the pipeline's own intermediate on the same inputs
    from reflecting_reality_amd import program
    path = lambda k: os.path.join(a.out, info["manifest"]["files"][k])
    pe, ne = pipe.encode_prompt(prompts, 1, True, negative_prompt=neg)
    want_pe = torch.cat([ne, pe]).to(dev, te.prec.act).contiguous()
    enc = program.Program(path("encode_prompt"), dev)
    enc.write("input_ids", ids)
    enc.run()
    torch.cuda.synchronize()
    print("  encode_prompt program == pipe.encode_prompt:", torch.equal(enc.buffer("prompt_embeds", te.prec.act).view(want_pe.shape), want_pe))
    enc.close()
    want_cond = pipe.build_conditioning(planes(image), planes(mask), depth, 512, 512, 4, 1, True, noise)
    cond = program.Program(path("conditioning"), dev)
    for k, t in (("image_u8", image), ("mask_u8", mask), ("depth", depth), ("cond_noise", noise)):
        cond.write(k, t)
    cond.run()
    torch.cuda.synchronize()
    print("  conditioning program == pipe.build_conditioning:", torch.equal(cond.buffer("cond", torch.float32).view(want_cond.shape), want_cond))
    cond.close()
    lat = pipe(image=planes(image), mask=planes(mask), output_type="latent", **kw).images.float().contiguous()
    dec = program.Program(path("decode"), dev)
    dec.write("latents", lat)
    dec.run()
    torch.cuda.synchronize()
    print("  decode program on the pipeline's latents == pipeline image:", bool(np.array_equal(dec.buffer("image_u8").view(want.shape).cpu().numpy(), want)))
    dec.close()
    shutil.rmtree(a.out)


if a.call:
    whole_call()
    sys.exit(0)
inp = {k: v.to(dev) for k, v in synth.pipeline_inputs(4, 512, 512, seed=1234, cross_dim=768).items()}
kw = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
          depth=inp["depth"], num_inference_steps=a.steps, guidance_scale=7.5, latents=inp["latents"], output_type="latent",
          brushnet_conditioning_scale=1.0, height=512, width=512, conditioning_noise=inp["vae_noise"])
tm = {}
ref = pipe(**kw, _timing=tm).images.float().cpu()          # the pipeline's own loop: eager first step, capture, replays
tm = {}
ref2 = pipe(**kw, _timing=tm).images.float().cpu()
torch.cuda.synchronize()
print(f"pipeline (hipGraph on two streams): {tm['denoise_start'].elapsed_time(tm['denoise_end']) / a.steps:.3f} ms per denoise step; "
      f"repeatable: {torch.equal(ref, ref2)}")
pipe._graph_state = None
t0 = time.time()
info = pipe.export_denoise_step(a.out, **kw)
print(f"exported in {time.time() - t0:.1f} s: {info['calls']} calls, {info['buffers']} buffers, file {info['bytes'] / 1e9:.3f} GB "
      f"({info['const_bytes'] / 1e9:.3f} GB constants, {info['workspace_bytes'] / 1e9:.3f} GB workspace); entries {info['entries']}")
print("exporting run equals the plain run:", torch.equal(info["result"].images.float().cpu(), ref))
exe = "/tmp/denoise_host"
libdir = os.path.join(ROOT, "reflecting-reality_amd", "lib")
subprocess.run(["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}",
                os.path.join(ROOT, "examples", "c_host", "denoise_host.c"), f"-L{libdir}", "-lmfhip", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe], check=True)
inp["latents"].float().cpu().contiguous().numpy().tofile("/tmp/lat_in.bin")
del pipe
torch.cuda.empty_cache()
torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
runtimes = {"ROCm 7.2 runtime (/opt/rocm/lib)": f"{libdir}:/opt/rocm/lib:", "the torch wheel's runtime": f"{libdir}:{torch_lib}:/opt/rocm/lib:"}
for (label, path), extra in [(r, e) for r in list(runtimes.items())[:1] for e in ([], ["--graph"])]:
    env = dict(os.environ, LD_LIBRARY_PATH=path + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, a.out, "/tmp/lat_in.bin", "/tmp/lat_out.bin"] + extra, capture_output=True, text=True, timeout=1200, env=env)
    print(f"[{label} {' '.join(extra)}]", out.stdout.strip().splitlines()[-1] if out.returncode == 0 else out.stdout + out.stderr)
    if out.returncode == 0:
        got = torch.from_numpy(np.fromfile("/tmp/lat_out.bin", dtype=np.float32)).view(ref.shape)
        print("   C host latents == pipeline latents (bitwise):", torch.equal(got, ref), "max |diff|", float((got - ref).abs().max()))
# the same program replayed from THIS process (torch's streams, torch's graph capture): separates what the program's structure
# costs from what the C host's streams / instantiation cost
from reflecting_reality_amd import program  # noqa: E402
prog = program.Program(a.out, dev)
lat0 = prog.buffer("latents", torch.float32).clone()
for mode in ("eager", "graph"):
    prog.buffer("latents", torch.float32).copy_(lat0)
    g = None
    if mode == "graph":
        prog.run()
        prog.buffer("latents", torch.float32).copy_(lat0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            prog.run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        g.replay() if g is not None else prog.run()
    e1.record()
    torch.cuda.synchronize()
    print(f"[python host, {mode}] {e0.elapsed_time(e1) / 20:.3f} ms per program run")
prog.close()
os.remove(a.out)
