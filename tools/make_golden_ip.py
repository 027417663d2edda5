"""Golden fixtures of the 'ip_adapter' normals mode, from the IMPORTED REFERENCE (its FreqEncoder, NormalProjModel, IPAttnProcessor2_0,
Attention, UNet2DConditionModel, BrushNetModel and DDIMScheduler), in the style of tools/make_golden.py.

Runs only in the build container (needs /root/reference); nothing under tests/, bench.py or the package
reads the reference at run time.  Writes, under tests/golden/:

  ip_adapter_tiny.npz         (a) FreqEncoder and NormalProjModel outputs for 3 normals;
                              (b) one Attention layer under IPAttnProcessor2_0 at num_tokens 1 and 4 (inputs, weights, outputs);
                              (c) the TINY_UNET's output for [2, 78, 32] prompts at two timesteps, IP processors on every attn2;
                              (d) the latents of a 4-step DDIM run done the way MirrorFusionModel.forward does it
                                  (train_brushnet_mirror.py:858-888: BrushNet gets the 77 text tokens, the UNet gets text + normal token;
                                  CFG 7.5, batch 1, 16 x 16);
                              (f) the mean normal over a mask (dataset.py:173-180, restated here: that module imports h5py / torchvision,
                                  which this image lacks);
                              and the seeded IP weights themselves ("ipw/<i>.to_k_ip.weight", ..., "proj/proj.0.weight", ...: what an
                              ip-adapter.bin of this model holds).
  keys_ip_adapter_tiny.json   the reference's attn_processors keys in ITS order, and the key -> shape tables of the checkpoint.
  ip_adapter_envelope.json    (e) the reference's own bf16 and fp16 deviation on (c) and (d), as tools/make_bf16_envelope.py records it.

    python tools/make_golden_ip.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden as MG  # noqa: E402  (sets up the reference import path + shim)
from make_golden import BrushNetModel, DDIMScheduler, GOLD, R, synth  # noqa: E402

sys.path.insert(0, "/root/reference/MirrorFusion/examples/brushnet")
from ip_adapter.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0  # noqa: E402
from ip_adapter.ip_adapter import FreqEncoder, NormalProjModel  # noqa: E402
from diffusers.models.attention_processor import Attention  # noqa: E402

torch.set_grad_enabled(False)
CROSS = R.TINY_UNET["cross_attention_dim"]
IP_SCALE, NUM_TOKENS = 1.0, 4            # train_brushnet_mirror.py leaves both at IPAttnProcessor2_0's defaults


def seeded(shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def install_ip(unet, seed=300):
    """train_brushnet_mirror.py:1100-1122: IPAttnProcessor2_0 on every attn2, AttnProcessor2_0 on every attn1; here with seeded
    to_k_ip / to_v_ip instead of copies of to_k / to_v, so that a swapped pair or a wrong layer shows."""
    procs = {}
    for i, name in enumerate(unet.attn_processors.keys()):
        if name.endswith("attn1.processor"):
            procs[name] = AttnProcessor2_0()
            continue
        if name.startswith("mid_block"):
            hidden = unet.config.block_out_channels[-1]
        elif name.startswith("up_blocks"):
            hidden = list(reversed(unet.config.block_out_channels))[int(name[len("up_blocks.")])]
        else:
            hidden = unet.config.block_out_channels[int(name[len("down_blocks.")])]
        p = IPAttnProcessor2_0(hidden_size=hidden, cross_attention_dim=CROSS, scale=IP_SCALE, num_tokens=NUM_TOKENS)
        p.to_k_ip.weight.copy_(seeded(p.to_k_ip.weight.shape, seed + 2 * i, CROSS ** -0.5))
        p.to_v_ip.weight.copy_(seeded(p.to_v_ip.weight.shape, seed + 2 * i + 1, CROSS ** -0.5))
        procs[name] = p
    unet.set_attn_processor(procs)
    return torch.nn.ModuleList(unet.attn_processors.values())


def normal_models(seed=400):
    fe = FreqEncoder(input_dim=3, max_freq_log2=5, N_freqs=32, log_sampling=True, include_input=False, periodic_fns=(torch.sin, torch.cos))
    proj = NormalProjModel(cross_attention_dim=CROSS, normals_embeddings_dim=192)
    proj.proj[0].weight.copy_(seeded(proj.proj[0].weight.shape, seed, 192 ** -0.5))
    proj.proj[0].bias.copy_(seeded(proj.proj[0].bias.shape, seed + 1, 0.1))
    return fe, proj


def normals3():
    n = torch.tensor([[0.0, 0.0, 1.0], [0.6, -0.48, 0.64], [-0.7071068, 0.7071068, 0.0]])
    return (n / n.norm(dim=-1, keepdim=True))[:, None, :]            # [3, 1, 3]


def layer_case(num_tokens, seed):
    """(b): one reference Attention (query 64, cross 32, 8 heads of 8: a head dim of the flash kernels) under
    IPAttnProcessor2_0(scale 0.7, num_tokens)."""
    attn = Attention(query_dim=64, cross_attention_dim=CROSS, heads=8, dim_head=8, bias=False).eval()
    g = torch.Generator().manual_seed(seed)
    for p in attn.parameters():
        p.copy_(torch.randn(p.shape, generator=g) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
    proc = IPAttnProcessor2_0(hidden_size=64, cross_attention_dim=CROSS, scale=0.7, num_tokens=num_tokens)
    proc.to_k_ip.weight.copy_(torch.randn(64, CROSS, generator=g) * CROSS ** -0.5)
    proc.to_v_ip.weight.copy_(torch.randn(64, CROSS, generator=g) * CROSS ** -0.5)
    attn.set_processor(proc)
    hs, ehs = torch.randn(2, 24, 64, generator=g), torch.randn(2, 74 + num_tokens, CROSS, generator=g)
    out = attn(hs, encoder_hidden_states=ehs)
    d = {f"layer{num_tokens}_{k}": v.numpy() for k, v in attn.state_dict().items() if not k.startswith("processor")}
    d.update({f"layer{num_tokens}_to_k_ip.weight": proc.to_k_ip.weight.numpy(), f"layer{num_tokens}_to_v_ip.weight": proc.to_v_ip.weight.numpy(),
              f"layer{num_tokens}_hidden_states": hs.numpy(), f"layer{num_tokens}_encoder_hidden_states": ehs.numpy(),
              f"layer{num_tokens}_out": out.numpy()})
    return d


def unet_inputs():
    g = torch.Generator().manual_seed(43)
    return torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 77 + 1, CROSS, generator=g)


def denoise(unet, brushnet, cond, pe, token, latents, steps=4, guidance=7.5, dtype=torch.float32):
    """The loop of pipeline_brushnet.py:1250-1332 with MirrorFusionModel.forward's wiring (train_brushnet_mirror.py:858-888): BrushNet
    reads the text tokens, the UNet reads cat([text, ip token], 1)."""
    sched = DDIMScheduler(**{k: v for k, v in R.SD15_SCHED.items() if k != "skip_prk_steps"})
    sched.set_timesteps(steps)
    pe_u = torch.cat([pe, torch.cat([token, token])], 1)              # get_normal_embeds: the same token in both CFG halves
    trace = []
    for t in sched.timesteps:
        x_in = sched.scale_model_input(torch.cat([latents] * 2), t)
        down, mid, up = brushnet(x_in.to(dtype), t, encoder_hidden_states=pe.to(dtype), brushnet_cond=cond.to(dtype), return_dict=False)
        eps = unet(x_in.to(dtype), t, encoder_hidden_states=pe_u.to(dtype), down_block_add_samples=list(down), mid_block_add_sample=mid,
                   up_block_add_samples=list(up), return_dict=False)[0].float()
        eu, ec = eps.chunk(2)
        latents = sched.step(eu + guidance * (ec - eu), t, latents, return_dict=False)[0]
        trace.append(latents.clone())
    return trace


def stats(got, ref):
    e = (got.float() - ref.float()).abs()
    return dict(linf=float(e.max()), mean=float(e.mean()), ref_absmax=float(ref.abs().max()), ref_absmean=float(ref.abs().mean()))


def main():
    out, keys = {}, {}
    # ---- (a) ----
    fe, proj = normal_models()
    n3 = normals3()
    enc = fe(n3)
    out["normals3"], out["freq_encoded"], out["normal_tokens"] = n3.numpy(), enc.numpy(), proj(enc).numpy()
    for k, v in proj.state_dict().items():
        out["proj/" + k] = v.numpy()
    # ---- (b) ----
    out.update(layer_case(1, 501))
    out.update(layer_case(4, 504))
    # ---- (c) ----
    unet = MG.build_unet(R.TINY_UNET)
    usd, _ = MG.load_synth(unet, 0)
    adapter = install_ip(unet)
    for k, v in adapter.state_dict().items():
        out["ipw/" + k] = v.numpy()
    keys["attn_processors"] = list(unet.attn_processors.keys())
    keys["ip_adapter"] = {k: list(v.shape) for k, v in adapter.state_dict().items()}
    keys["image_proj"] = {k: list(v.shape) for k, v in proj.state_dict().items()}
    x, ehs = unet_inputs()
    eps = {t: unet(x, t, encoder_hidden_states=ehs, return_dict=False)[0] for t in (501, 21)}
    for t, e in eps.items():
        out[f"unet_eps_t{t}"] = e.numpy()
    # ---- (d) ----
    brushnet = BrushNetModel.from_unet(MG.build_unet(R.TINY_UNET), conditioning_channels=6, load_weights_from_unet=False).eval()
    bsd, _ = MG.load_synth(brushnet, 1)
    vae = MG.build_vae(R.TINY_VAE)
    vsd, _ = MG.load_synth(vae, 2)
    inp = synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=CROSS, vae_scale=2)
    cond = R.build_conditioning(vsd, R.TINY_VAE, inp["image"], inp["mask"], inp["depth"], inp["vae_noise"])
    pe = torch.cat([inp["negative_prompt_embeds"], inp["prompt_embeds"]])
    token = proj(fe(n3[1:2]))                                         # [1, 1, 32]: the second of the three normals
    trace = denoise(unet, brushnet, cond, pe, token, inp["latents"])
    for i, l in enumerate(trace):
        out[f"pipeline_latents_{i}"] = l.numpy()
    out["pipeline_vae_noise"] = inp["vae_noise"].numpy()
    out["pipeline_cond"] = cond.numpy()
    # ---- (f): dataset.py:173-180 ----
    g = torch.Generator().manual_seed(77)
    nm = (torch.rand(24, 20, 3, generator=g) * 2.0 - 1.0).numpy().astype(np.float32)
    mk = ((torch.rand(24, 20, generator=g) > 0.6).float() * 255.0).numpy().astype(np.float32)
    mean = np.mean(np.copy(nm)[mk > 0], axis=0)
    out["mean_normal_map"], out["mean_normal_mask"] = nm, mk
    out["mean_normal"] = torch.tensor(mean / np.linalg.norm(mean), dtype=torch.float32).unsqueeze(0).numpy()
    # ---- (e) ----
    env = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        e = env[name] = {}
        for m in (unet, brushnet):
            m.to(dt)
        for t in (501, 21):
            e[f"ip_tiny/unet_eps_t{t}"] = stats(unet(x.to(dt), t, encoder_hidden_states=ehs.to(dt), return_dict=False)[0], eps[t])
        for i, l in enumerate(denoise(unet, brushnet, cond, pe, token, inp["latents"], dtype=dt)):
            e[f"ip_tiny/pipeline_latents_{i}"] = stats(l, trace[i])
        for m in (unet, brushnet):
            m.to(torch.float32)
    np.savez_compressed(os.path.join(GOLD, "ip_adapter_tiny.npz"), **out)
    with open(os.path.join(GOLD, "keys_ip_adapter_tiny.json"), "w") as f:
        json.dump(keys, f, indent=1)
    with open(os.path.join(GOLD, "ip_adapter_envelope.json"), "w") as f:
        json.dump(env, f, indent=1)
    print(f"wrote ip_adapter_tiny.npz ({os.path.getsize(os.path.join(GOLD, 'ip_adapter_tiny.npz'))} bytes), {len(keys['attn_processors'])} processors")
    print(json.dumps(env, indent=1)[:1200])


if __name__ == "__main__":
    main()
