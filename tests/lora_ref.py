"""Reference arithmetic of the LoRA tests (a plain helper module, like gemm_ref.py): the merge in float64, the per-element bound of
mf_lora_merge's contract, and the host-merged state dict of a fixture adapter."""
import json

import torch

from reflecting_reality_amd import lora, synth


def merge64(base, terms):
    """base [rows, cols] fp32, terms [(up [rows, r], down [r, cols], coef)] -> (float64 result, float64 magnitude sum
    |base| + sum |coef| sum_j |up||down|).  coef enters at its fp32 value, as the device reads it."""
    out, mag = base.double().clone(), base.double().abs()
    for up, down, coef in terms:
        c = float(torch.tensor(coef, dtype=torch.float32))
        out += c * (up.double() @ down.double())
        mag += abs(c) * (up.double().abs() @ down.double().abs())
    return out, mag


def bound(terms, mag):
    """|out - ref64| <= (R + 4) * 2^-24 * mag, R the sum of the ranks: one rounding per fma of the rank loops (R of them, each at most
    half an ulp of a partial sum bounded by mag), one per term's scaled add, the final rounding of the float64 reference to fp32 and
    the fp32 coef product are covered by the 4."""
    r = sum(int(up.shape[1]) for up, _, _ in terms)
    return (r + 4) * 2.0 ** -24 * mag


def plan_of(G, case):
    return [(m, int(r), a) for m, r, a in json.loads(str(G[f"{case}_plan"]))]


def adapter_of(G, case, shapes, prefix=""):
    """The fixture's adapter (diffusers format) and its alphas, regenerated from the recipe recorded in lora_tiny.npz."""
    return synth.lora_adapter(plan_of(G, case), shapes, int(G[f"{case}_seed"]), float(G[f"{case}_gain"]), prefix=prefix)


def host_merged(sd, shapes, capable, adapters, scale=1.0):
    """{name: fp32 tensor}: sd with adapters = [(state dict, alphas, weight)] merged in float64 at `scale` and rounded to fp32."""
    terms = {}
    for asd, alphas, weight in adapters:
        groups = lora.group_keys(asd, alphas)
        entries = dict(list(groups["unet"].items()) + list(groups["text_encoder"].items()) + list(groups[""].items()))
        for m, (down, up, coef) in lora.resolve(entries, shapes, capable).items():
            terms.setdefault(m, []).append((down, up, float(weight) * float(scale) * coef))
    return lora.merge_host(sd, terms)
