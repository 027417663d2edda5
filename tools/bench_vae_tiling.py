"""Tiled VAE decode / encode on the device: the grouped schedule against one tile per pass and against the untiled pass.

SD1.5 VAE with the bench's synthetic weights (sample_size 512: 64 x 64-latent tiles, overlap 48 latents / 384 pixels), bf16, one image,
at 1024 x 1024 and 2048 x 2048 pixels.  Three schedules of the SAME call, alternated in one process after every shape was warmed:
  grouped     enable_tiling(), tile_batch at its default: the tiles of one shape stacked on the batch axis, one pass per shape
  one-by-one  enable_tiling(), tile_batch = 1: the reference's loop, one pass per tile
  untiled     tiling off (only up to --untiled-max pixels; beyond it the unfused d = 512 attention of the mid block materialises
              S x S scores: 17 GB at 2048 x 2048)
Each timing is a device-event window around `--calls` calls, repeated `--repeats` times; the median and the spread (max - min) of the
repeats are reported.  The crop and blend launches of a tiled call are replayed alone on buffers of the same shapes to give their share.
The tiled and untiled results differ by design (tiling changes the result, in the reference too); the two tiled schedules are compared.
Not a bench.py leg; there is no threshold.  Writes profiles/vae_tiling_bench.txt.

usage: python tools/bench_vae_tiling.py [--sizes 1024 2048] [--repeats 5] [--calls 2] [--untiled-max 1024]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="calls per timed window")
    ap.add_argument("--untiled-max", type=int, default=1024, help="largest size at which the untiled pass is run")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_tiling_bench.txt"))
    a = ap.parse_args()
    from reflecting_reality_amd import AutoencoderKL, hip, synth
    from reflecting_reality_amd.configs import SD15_VAE
    from reflecting_reality_amd.models import vae_tile_plan
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_tiling.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    hip.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    vae = AutoencoderKL(dict(SD15_VAE, sample_size=512), precision=a.precision, device=dev)
    vae.load_state_dict(synth.state_dict_for(vae.param_shapes(), 2))
    vae._src = None
    default_tb = vae.tile_batch

    def window(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.calls):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / a.calls

    def data_movement(x, encode):
        """The crop-pack and blend launches of one tiled call, alone, on buffers of the call's shapes."""
        levels = len(vae.config["block_out_channels"]) - 1
        if encode:
            plan = vae_tile_plan(x.shape[2], x.shape[3], vae.tile_sample_min_size, vae.tile_overlap_factor, 1, 2 ** levels, vae.tile_latent_min_size)
            c = 2 * vae.config["latent_channels"]
            c_pad, ld = vae.cin_pad, (c + 3) // 4 * 4
            out = torch.empty(1, plan["out_h"], plan["out_w"], ld, device=dev)
        else:
            plan = vae_tile_plan(x.shape[2], x.shape[3], vae.tile_latent_min_size, vae.tile_overlap_factor, 2 ** levels, 1, vae.tile_sample_min_size)
            c_pad, ld, c = vae.lat_pad, 4, vae.config["out_channels"]
            out = torch.empty(1, c, plan["out_h"], plan["out_w"], device=dev)
        stacks = {(t["i"], t["j"]): torch.empty(1, t["h"], t["w"], c_pad, dtype=vae.prec.act, device=dev) for t in plan["tiles"]}
        done = {(t["i"], t["j"]): torch.randn(1, t["out_h"], t["out_w"], ld, device=dev) for t in plan["tiles"]}

        def run():
            for t in plan["tiles"]:
                hip.crop_pack_nhwc(x, t["y0"], t["x0"], t["h"], t["w"], stacks[(t["i"], t["j"])], 0)
            for t in plan["tiles"]:
                i, j = t["i"], t["j"]
                hip.vae_tile_blend(done[(i, j)], done.get((i - 1, j)), done.get((i, j - 1)), plan["blend_extent"], plan["row_limit"], c, out,
                                   t["oy"], t["ox"], nhwc=encode)
        return run, plan

    say(f"tiled VAE, SD1.5 VAE (sample_size 512), {a.precision}, batch 1, {torch.cuda.get_device_name(0)}")
    say(f"median ms per call over {a.repeats} repeats of {a.calls} calls, schedules alternated (spread = max - min over the repeats); "
        f"tile_batch default {default_tb}")
    g = torch.Generator().manual_seed(3)
    for size in a.sizes:
        for what in ("decode", "encode"):
            encode = what == "encode"
            x = (torch.rand(1, 3, size, size, generator=g) * 2 - 1 if encode else torch.randn(1, 4, size // 8, size // 8, generator=g)).to(dev)
            call = (lambda: vae._moments(x)) if encode else (lambda: vae.decode(x, return_dict=False)[0])

            def grouped():
                vae.enable_tiling(); vae.tile_batch = default_tb
                return call()

            def one_by_one():
                vae.enable_tiling(); vae.tile_batch = 1
                return call()

            def untiled():
                vae.disable_tiling()
                return call()
            schedules = [("grouped", grouped), ("one-by-one", one_by_one)]
            if size <= a.untiled_max:
                schedules.append(("untiled", untiled))
            move, plan = data_movement(x, encode)
            schedules.append(("crop + blend launches alone", move))
            results, refused = {}, {}
            for name, fn in schedules:                     # warm every shape (and learn what the library refuses)
                try:
                    results[name] = fn()
                    torch.cuda.synchronize()
                except hip.MfhipError as e:
                    refused[name] = str(e).splitlines()[0][:160]
            times = {name: [] for name, _ in schedules if name not in refused}
            for _ in range(a.repeats):
                for name, fn in schedules:
                    if name not in refused:
                        times[name].append(window(fn))
            shapes = sorted({(t["h"], t["w"]) for t in plan["tiles"]}, reverse=True)
            say()
            say(f"{what} at {size} x {size} pixels: {len(plan['tiles'])} tiles in {len(shapes)} shapes {shapes}, output {plan['out_h']} x {plan['out_w']}")
            for name, _ in schedules:
                if name in refused:
                    say(f"  {name:28s} refused: {refused[name]}")
                else:
                    ts = times[name]
                    say(f"  {name:28s} {statistics.median(ts):9.3f} ms   spread {max(ts) - min(ts):7.3f}")
            med = {n: statistics.median(ts) for n, ts in times.items()}
            if "grouped" in med and "one-by-one" in med:
                say(f"  one-by-one / grouped = {med['one-by-one'] / med['grouped']:.2f}; crop + blend share of the grouped call = "
                    f"{100 * med['crop + blend launches alone'] / med['grouped']:.1f} %")
                d = (results["grouped"].float() - results["one-by-one"].float()).abs().max().item()
                say(f"  grouped vs one-by-one results: max abs difference {d:.3e} (|result| max {results['grouped'].float().abs().max().item():.2f})")
            if "untiled" in med:
                say(f"  untiled / grouped = {med['untiled'] / med['grouped']:.2f} (different results by design: tiling changes the image)")
            elif size > a.untiled_max:
                say("  untiled: not measured at this size")
            del results
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
