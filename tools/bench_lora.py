"""Writes profiles/lora_bench.txt: what changing a LoRA adapter or its scale costs on the full-size SD1.5 UNet (synth weights, bf16).

    python tools/bench_lora.py [--out FILE] [--no-denoise]

Two adapters (synth tensors): A, rank 16 on the attention projections (to_q / to_k / to_v / to_out.0); B, rank 64 on every layer the
reference can adapt (its LoRACompatibleConv / LoRACompatibleLinear layers outside the time embedding).  Per adapter, median of 5 with
the range, host clock around work that ends in a device synchronise:
  load           load_attn_procs: parse, check, upload up / down, stash the fp32 base of the targeted weights, build the device tables
  first merge    the merge launch and the re-derivation of the targeted layouts
  re-merge       the same at another scale (0.7 <-> 0.3)
  unfuse         back to the base layouts (fuse_lora first, untimed)
  mf_lora_merge  the launch alone, device events; bytes moved (base read, out written, the factors once) and the apparent bandwidth
  host route     what the device route replaces: W + coef * up @ down in torch on the CPU for every targeted weight, then load_state_dict
                 (the whole UNet is uploaded and derived again), in this process
Then the 50-step DDIM denoise loop at batch 4 x 512 x 512 (device events) with no adapter, with adapter A fused, and with none again, 5
calls each after 2 warm-up calls: the step reads the same layouts, so the two must agree within the run-to-run range.
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reflecting_reality_amd import UNet2DConditionModel, hip, lora, synth  # noqa: E402
from reflecting_reality_amd.configs import SD15_UNET  # noqa: E402

DEV = torch.device("cuda", 0)
OUT = os.path.join(ROOT, "profiles", "lora_bench.txt")
_lines = []


def emit(line=""):
    print(line, flush=True)
    _lines.append(line)
    with open(OUT, "w") as f:                      # kept as it grows: a run that is cut short leaves what it measured
        f.write("\n".join(_lines) + "\n")


def timed(fn, n=5, before=None):
    ts = []
    for _ in range(n):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def fmt(ts):
    return f"median {statistics.median(ts):10.2f} ms   min {min(ts):10.2f}   max {max(ts):10.2f}"


def adapter(unet, which):
    shapes = unet.param_shapes()
    if which == "A":
        mods = [m for m in unet.lora_modules() if ".attn" in m and m.rsplit(".", 1)[-1] in ("to_q", "to_k", "to_v", "0")]
        rank = 16
    else:
        mods = [m for m in unet.lora_modules() if not m.startswith(("conv_in", "conv_out", "time_embedding.", "add_embedding."))]
        rank = 64
    return synth.lora_adapter([(m, rank, float(rank)) for m in mods], shapes, 7, 0.2, prefix="unet."), mods, rank


def host_route(unet, sd, asd, alphas, scale):
    groups = lora.group_keys(asd, alphas)
    found = lora.resolve(groups["unet"], unet.param_shapes(), unet.lora_modules())
    merged = dict(sd)
    for m, (down, up, coef) in found.items():
        w = sd[m + ".weight"]
        merged[m + ".weight"] = (w.reshape(w.shape[0], -1) + (coef * scale) * (up @ down)).reshape(w.shape)
    unet.load_state_dict(merged)


def main():
    out = OUT
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    globals()["OUT"] = out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hip.load()
    emit("LoRA adapters on the full-size SD1.5 UNet (synth weights, bf16), one MI355X; tools/bench_lora.py")
    emit(f"device: {torch.cuda.get_device_name(0)}; host threads: {torch.get_num_threads()}")
    emit()
    unet = UNet2DConditionModel(dict(SD15_UNET), precision="bf16", device=DEV)
    sd = synth.state_dict_for(unet.param_shapes(), 0)
    t = timed(lambda: unet.load_state_dict(sd), n=3)
    emit(f"load_state_dict of the whole UNet (no adapter), for scale: {fmt(t)}   (3 runs)")
    for which in ("A", "B"):
        (asd, alphas), mods, rank = adapter(unet, which)
        nw = sum(sd[m + ".weight"].numel() for m in mods)
        emit()
        emit(f"adapter {which}: rank {rank} on {len(mods)} weights, {nw / 1e6:.1f} M of the UNet's {sum(v.numel() for v in sd.values()) / 1e6:.1f} M parameters")
        emit(f"  load            {fmt(timed(lambda: unet.load_attn_procs(asd, network_alphas=alphas), before=unet.unload_lora))}")
        first = timed(lambda: unet._lora_sync(0.7), before=lambda: (unet.unload_lora(), unet.load_attn_procs(asd, network_alphas=alphas)))
        emit(f"  first merge     {fmt(first)}")
        flip = iter([0.3, 0.7] * 8)
        remerge = timed(lambda: unet._lora_sync(next(flip)))
        emit(f"  re-merge        {fmt(remerge)}")
        emit(f"  unfuse          {fmt(timed(unet.unfuse_lora, before=lambda: unet.fuse_lora(0.7)))}")
        tables = unet._lora_state().tables
        ev = []
        for i in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            hip.lora_merge(tables)
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ev.append(a.elapsed_time(b))
        med = statistics.median(ev)
        emit(f"  mf_lora_merge   {fmt(ev)}   {tables.bytes / 1e9:.3f} GB moved, {tables.bytes / med / 1e9:.2f} TB/s apparent "
             f"({tables.ntargets} targets, {tables.tiles} tiles, one launch; 2 warm-up launches)")
        unet.unload_lora()
        host = timed(lambda: host_route(unet, sd, asd, alphas, 0.7))
        emit(f"  host route      {fmt(host)}")
        verdict = "beats" if max(remerge) < min(host) else "does NOT beat"
        emit(f"  the device re-merge {verdict} the host route outside the spread: {statistics.median(host) / statistics.median(remerge):.1f} x on the medians")
        unet.load_state_dict(sd)
    del unet
    if "--no-denoise" in sys.argv:
        return
    import bench
    emit()
    emit("50-step DDIM denoise loop, batch 4 x 512 x 512, bf16 (device events, ms), no adapter, adapter A fused at 0.7, no adapter again;")
    emit("2 warm-up calls per state, then 5 timed calls each")
    pipe, _ = bench.build_pipeline("bf16", DEV)
    pipe.unet._src = sd
    inp = synth.pipeline_inputs(4, 512, 512)
    (asd, alphas), _, _ = adapter(pipe.unet, "A")
    times = {"none": [], "fused": [], "none (again, last: drift check)": []}
    for state in times:                            # a state at a time: changing the weights captures the step graph again
        if state == "fused":
            pipe.load_lora_weights({**asd, **{k: torch.tensor(v) for k, v in alphas.items()}})
            pipe.fuse_lora(lora_scale=0.7)
        for rnd in range(7):
            timing = {}
            pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
                 depth=inp["depth"], num_inference_steps=50, guidance_scale=7.5, latents=inp["latents"], output_type="latent", height=512,
                 width=512, _timing=timing)
            torch.cuda.synchronize()
            if rnd >= 2:
                times[state].append(timing["denoise_start"].elapsed_time(timing["denoise_end"]))
        if state == "fused":
            pipe.unload_lora_weights()
    for state in times:
        emit(f"  {state:32s} {fmt(times[state])}")
    lo, hi = (min(times["none"]), max(times["none"])), (min(times["fused"]), max(times["fused"]))
    emit(f"  the ranges {'overlap' if lo[0] <= hi[1] and hi[0] <= lo[1] else 'do NOT overlap'}: a fused adapter costs nothing per step")


if __name__ == "__main__":
    main()
