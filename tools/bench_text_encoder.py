"""One encode of 8 prompts through the HIP CLIP text encoders: CLIP-L (12 layers) and a full-depth OpenCLIP bigG (32 layers),
synth weights, bf16 and f16x3, eager and replayed from a hipGraph; beside them the same transformers module's eager time on
torch-ROCm when transformers is importable.  Writes the table to stdout and to --out (default profiles/r07_text_encoder.txt).

    timeout 900 python tools/bench_text_encoder.py [--out FILE] [--models clip_l bigg]

Not on the timed path (bench.py feeds prompt_embeds): an encode is a few GFLOP once per prompt against ~125 TFLOP per image.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reflecting_reality_amd import synth  # noqa: E402
from reflecting_reality_amd.configs import CLIP_L_TEXT, OPENCLIP_BIGG_TEXT  # noqa: E402
from reflecting_reality_amd.text_encoder import CLIPTextModel, CLIPTextModelWithProjection  # noqa: E402

CONFIGS = {"clip_l": (CLIPTextModel, CLIP_L_TEXT), "bigg": (CLIPTextModelWithProjection, OPENCLIP_BIGG_TEXT)}
PROMPTS = ["a perfect plane mirror reflection of a wooden chair standing on a tiled floor", "a mug", "a red sofa next to a window",
           "a cat", "a mirror on the wall of a bathroom reflecting a towel", "a plant", "two books on a glass table", "a lamp"]
DEV = "cuda"


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_text_encoder.txt"))
    ap.add_argument("--models", nargs="*", default=list(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    lines = [f"CLIP text encoders, one encode of {len(PROMPTS)} prompts x 77 tokens, {torch.cuda.get_device_name(0)}, ms per encode",
             f"{'model':8s} {'precision':9s} {'eager':>9s} {'hipGraph':>9s}   (eager = model(ids) with host ids; hipGraph = embedding + layers + final LN replayed)"]
    for name in a.models:
        klass, cfg = CONFIGS[name]
        tok = synth.HashTokenizer(cfg["vocab_size"], 77, pad_token_id=None if cfg["eos_token_id"] == 2 else 0)
        ids = tok(PROMPTS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        sd = None
        for prec in ("bf16", "f16x3"):
            model = klass(dict(cfg), precision=prec, device=DEV)
            sd = sd or synth.state_dict_for(model.param_shapes(), 7)
            model.load_state_dict(sd)
            eager = timed(lambda: model(ids, output_hidden_states=True), a.iters)
            ids_dev = ids.to(DEV, torch.int32)
            model._stack(ids_dev)                                   # every GEMM shape tuned before the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                model._stack(ids_dev)
            graph = timed(g.replay, a.iters)
            lines.append(f"{name:8s} {prec:9s} {eager:9.3f} {graph:9.3f}")
            print(lines[-1], flush=True)
            del model, g
        try:
            import transformers
            tcfg = transformers.CLIPTextConfig(**cfg, bos_token_id=cfg["vocab_size"] - 2, pad_token_id=1)
            tklass = transformers.CLIPTextModelWithProjection if klass is CLIPTextModelWithProjection else transformers.CLIPTextModel
            with torch.no_grad():
                ref = tklass(tcfg).eval().to(DEV, torch.bfloat16)
                ms = timed(lambda: ref(ids.to(DEV), output_hidden_states=True), a.iters)
            lines.append(f"{name:8s} transformers {transformers.__version__} on torch-ROCm, bf16, eager (default-initialised weights): {ms:9.3f}")
            del ref
        except ImportError:
            lines.append(f"{name:8s} transformers is not importable on this box: no torch-ROCm comparison")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
