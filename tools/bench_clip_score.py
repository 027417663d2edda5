"""One CLIP_Similarity call on the device: openai/clip-vit-large-patch14 shapes (24 vision layers, 12 text layers), synth weights, bf16,
a batch of 4 uint8 512 x 512 device images and 4 captions.  Reports ms per call for the preprocessing alone (with the bytes it moves and
the resulting GB/s), the vision tower alone (patch matrix -> image_embeds), the whole metrics.clip_score (tokenising, both towers, the
score kernel and the read of the row), and the number of library entries one score launches; beside it transformers' CLIPModel in bf16
on the same device when transformers is importable.  Writes the table to stdout and to --out (default profiles/clip_score_bench.txt).

    timeout 900 python tools/bench_clip_score.py [--out FILE]

Not on bench.py's timed path: a score is computed once per generated image, after the denoise loop.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reflecting_reality_amd import hip, metrics, synth  # noqa: E402
from reflecting_reality_amd.configs import CLIP_L  # noqa: E402
from reflecting_reality_amd.image_encoder import CLIPModel  # noqa: E402

CAPTIONS = ["a perfect plane mirror reflection of a wooden chair standing on a tiled floor", "a mug", "a red sofa next to a window",
            "a mirror on the wall of a bathroom reflecting a towel"]
DEV = "cuda"
BATCH, SIZE = 4, 512


def timed(fn, iters, repeats=5):
    """Median and spread (min .. max) of `repeats` windows of `iters` calls each, ms per call; every shape is warmed first."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(out), min(out), max(out)


def count_entries(fn):
    """Library entries (mf_* calls that launch) of one fn(): hip._launch is the door of every entry but mf_gemm_conv, which
    hip.gemm_conv enters with its descriptor."""
    calls = []
    real, real_gemm = hip._launch, hip.gemm_conv
    hip._launch = lambda entry, *a: (calls.append(entry), real(entry, *a))[1]
    hip.gemm_conv = lambda *a, **kw: (calls.append("mf_gemm_conv"), real_gemm(*a, **kw))[1]
    try:
        fn()
    finally:
        hip._launch, hip.gemm_conv = real, real_gemm
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_score_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    model = CLIPModel(dict(CLIP_L), precision="bf16", device=DEV)
    model.load_state_dict(synth.state_dict_for(model.param_shapes(), 7))
    tok = synth.HashTokenizer(CLIP_L["text_config"]["vocab_size"], 77)
    images = torch.from_numpy(synth.images_u8(3, BATCH, SIZE, SIZE)).to(DEV)
    vis = model.vision
    patches = vis.preprocess(images)
    # bytes the preprocessing has to move: the uint8 images read once, the patch matrix written once (the intermediate image of the
    # horizontal pass stays out: it is the implementation's, not the algorithm's)
    nbytes = images.numel() + patches.numel() * patches.element_size()
    lines = [f"CLIP_Similarity, ViT-L/14 (24 + 12 layers), bf16, batch {BATCH} of {SIZE} x {SIZE} uint8 device images, {torch.cuda.get_device_name(0)}",
             f"ms per call: median (min .. max) of 5 windows of {a.iters} calls"]
    med, lo, hi = timed(lambda: vis.preprocess(images), a.iters * 5)
    lines.append(f"preprocess (resize 512 -> 224, crop, normalise, unfold)  {med:8.3f} ({lo:.3f} .. {hi:.3f})   {nbytes / 1e6:.2f} MB moved, "
                 f"{nbytes / med / 1e6:.1f} GB/s")
    med, lo, hi = timed(lambda: vis(patches=patches).image_embeds, a.iters)
    lines.append(f"vision tower (patch matrix -> image_embeds)              {med:8.3f} ({lo:.3f} .. {hi:.3f})")
    med, lo, hi = timed(lambda: metrics.clip_score(images, CAPTIONS, model, tok), a.iters)
    lines.append(f"metrics.clip_score (tokenise, both towers, score, read)  {med:8.3f} ({lo:.3f} .. {hi:.3f})")
    calls = count_entries(lambda: metrics.clip_score(images, CAPTIONS, model, tok))
    kinds = {k: calls.count(k) for k in sorted(set(calls))}
    lines.append(f"library entries of one score: {len(calls)}  " + ", ".join(f"{k} x {v}" for k, v in kinds.items()))
    print("\n".join(lines), flush=True)
    try:
        import transformers
        t, v = dict(CLIP_L["text_config"]), dict(CLIP_L["vision_config"])
        cfg = transformers.CLIPConfig(text_config=dict(t, bos_token_id=t["vocab_size"] - 2, pad_token_id=1), vision_config=v,
                                      projection_dim=CLIP_L["projection_dim"])
        ids = tok(CAPTIONS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.to(DEV)
        pv = torch.randn(BATCH, 3, 224, 224, device=DEV, dtype=torch.bfloat16)
        with torch.no_grad():
            ref = transformers.CLIPModel(cfg).eval().to(DEV, torch.bfloat16)
            med, lo, hi = timed(lambda: ref(input_ids=ids, pixel_values=pv).logits_per_image.float().cpu(), a.iters)
        lines.append(f"transformers {transformers.__version__} CLIPModel on torch-ROCm, bf16, eager, pixel_values already on the device (no PIL, no "
                     f"processor): {med:8.3f} ({lo:.3f} .. {hi:.3f})")
    except ImportError:
        lines.append("transformers is not importable on this box: no torch-ROCm comparison")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
