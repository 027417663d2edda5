"""The 'ip_adapter' normals mode end to end on the device, against what the imported reference computed (tests/golden/ip_adapter_tiny.npz,
keys_ip_adapter_tiny.json, ip_adapter_envelope.json: tools/make_golden_ip.py): the frequency encoder and the normal projection, the mean
normal over a mask, one attention layer under MfhipIPAttnProcessor on the reference's processor ABI, the tiny UNet with IP processors on
every attn2, and a 4-step pipeline run wired the way MirrorFusionModel.forward wires it (train_brushnet_mirror.py:858-888).

fp32 and f16x3 meet the absolute tolerances tests/test_models_gpu.py and tests/test_pipeline_gpu.py apply to the same tiny nets; bf16 and
fp16 stay inside the reference's own deviation in that dtype on these very cases, with tests/util.py's ENV_K_* factors."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import util  # noqa: E402
from reflecting_reality_amd import (DDIMScheduler, MfhipAttnProcessor, MfhipIPAttnProcessor, PNDMScheduler, StableDiffusionBrushNetPipeline,  # noqa: E402
                                    frontend, hip, models as M, program, synth)
from reflecting_reality_amd.configs import SD15_SCHED, TINY_UNET, TINY_VAE, TINY_XL_UNET, brushnet_config  # noqa: E402
from util import golden, keys, report  # noqa: E402

DEV = "cuda"
PRECS = ["fp32", "f16x3", "bf16", "fp16"]
TOL_UNET = dict(atol=2e-4, rtol=2e-4)            # tests/test_models_gpu.py TOL
TOL_PIPE = dict(atol=1e-3)                       # tests/test_pipeline_gpu.py PREC_TOL
G = golden("ip_adapter_tiny.npz")
with open(os.path.join(util.GOLD, "ip_adapter_envelope.json")) as _f:
    ENV = json.load(_f)
_cache = {}


def check_ip(name, got, ref, prec, tol, key):
    """util.check with this feature's own envelope file: fp32-class precisions against atol / rtol `tol`; bf16 / fp16 against the
    reference's own deviation in that dtype on this case (ENV[prec][key]) with tests/util.py's factors, as util.report_env applies them."""
    if prec not in ENV:
        return report(name, got, ref, **tol)
    got, ref = torch.as_tensor(got).float().cpu(), torch.as_tensor(ref).float()
    err, env = (got - ref).abs(), ENV[prec][key]
    k_linf = util.ENV_K_LINF if ref.numel() >= util.ENV_SMALL_NUMEL else util.ENV_K_LINF_SMALL
    linf, mean = err.max().item(), err.mean().item()
    print(f"{name}: max_abs_err={linf:.3e} (reference {prec}: {env['linf']:.3e}) mean_abs_err={mean:.3e} (reference {prec}: {env['mean']:.3e}) "
          f"ENVRATIO linf {linf / env['linf']:.3f} mean {mean / env['mean']:.3f}")
    assert linf <= k_linf * env["linf"], f"{name}: L-inf {linf:.3e} > {k_linf} x the reference's {prec} envelope {env['linf']:.3e}"
    assert mean <= util.ENV_K_MEAN * env["mean"], f"{name}: mean error {mean:.3e} > {util.ENV_K_MEAN} x the reference's {prec} envelope {env['mean']:.3e}"
    return linf


def checkpoint():
    return {"image_proj": {k[len("proj/"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith("proj/")},
            "ip_adapter": {k[len("ipw/"):]: torch.from_numpy(G[k]) for k in G.files if k.startswith("ipw/")}}


def build(prec):
    if prec not in _cache:
        shapes = keys("tiny")
        unet = M.UNet2DConditionModel(dict(TINY_UNET), precision=prec, device=DEV)
        unet.load_state_dict(synth.state_dict_for(shapes["unet"], 0))
        image_proj = unet.load_ip_adapter(checkpoint())
        bn = M.BrushNetModel(dict(brushnet_config(TINY_UNET, 6)), precision=prec, device=DEV)
        bn.load_state_dict(synth.state_dict_for(shapes["brushnet"], 1))
        vae = M.AutoencoderKL(dict(TINY_VAE), precision=prec, device=DEV)
        vae.load_state_dict(synth.state_dict_for(shapes["vae"], 2))
        emb = frontend.NormalEmbedder(TINY_UNET["cross_attention_dim"], DEV, prec).load_state_dict(image_proj)
        _cache[prec] = (unet, bn, vae, emb)
    return _cache[prec]


def pipeline(prec, sched="ddim"):
    unet, bn, vae, emb = build(prec)
    s = (DDIMScheduler(**{k: v for k, v in SD15_SCHED.items() if k != "skip_prk_steps"}) if sched == "ddim" else PNDMScheduler(**SD15_SCHED))
    pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=bn, scheduler=s,
                                           safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           depth_conditioning_mode="concat", normals_conditioning_mode="ip_adapter")
    pipe.set_progress_bar_config(disable=True)
    pipe.normal_embedder = emb
    return pipe


def run(pipe, normal=None, embeds=None, steps=4, trace=None, seed=1234):
    inp = synth.pipeline_inputs(1, 16, 16, seed=seed, cross_dim=32, vae_scale=2)
    kw = dict(normals=normal) if embeds is None else dict(ip_adapter_image_embeds=embeds)
    cb = (lambda p, i, t, k: trace.append(k["latents"].float().cpu().clone()) or {}) if trace is not None else None
    return pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"], mask=inp["mask"],
                depth=inp["depth"], num_inference_steps=steps, guidance_scale=7.5, latents=inp["latents"].clone(), output_type="latent",
                height=16, width=16, conditioning_noise=torch.from_numpy(G["pipeline_vae_noise"]), callback_on_step_end=cb, **kw).images.float().cpu()


# ---- small pieces -----------------------------------------------------------------------------------------------------------------

def test_freq_encode_against_the_reference_encoder():
    """Arguments x f reach 32 (|x| <= 1, f <= 2^5).  Both sides form them in fp32: a relative error of 2^-23 of the argument moves
    sin / cos by at most 32 * 2^-23; each side then rounds its sin / cos (|.| <= 1) to fp32, 2^-23 for the two together."""
    n = torch.from_numpy(G["normals3"]).to(DEV)
    got = hip.freq_encode(n, 32, 5.0)
    assert tuple(got.shape) == (3, 1, 192)
    report("freq_encode", got, G["freq_encoded"], atol=32 * 2.0 ** -23 + 2.0 ** -23)
    # the layout: [sin(x f_0) (3), cos(x f_0) (3), sin(x f_1) (3), ...] with f_0 = 1
    assert torch.allclose(got[:, 0, :3].cpu(), torch.sin(torch.from_numpy(G["normals3"])[:, 0]), atol=1e-6)
    assert torch.allclose(got[:, 0, 3:6].cpu(), torch.cos(torch.from_numpy(G["normals3"])[:, 0]), atol=1e-6)


@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16"])
def test_normal_embedder(prec):
    """Linear(192, C) + erf-GELU over the encoding, in fp32 whatever the storage dtype: 192 products of |.| <= 1 encodings with
    weights ~ 192^-1/2, the encoder's 4e-6 carried through — 2e-5 absolute on tokens of size ~1; a 16-bit storage dtype rounds the
    result once more (2^-8 / 2^-11 relative)."""
    emb = build(prec)[3]
    tok = emb(torch.from_numpy(G["normals3"]))
    assert tuple(tok.shape) == (3, 1, 32) and tok.dtype == emb.prec.act
    rel = {"bf16": 2.0 ** -8}.get(prec, 0.0)
    report(f"normal tokens[{prec}]", tok, G["normal_tokens"], atol=2e-5, rtol=rel)
    assert emb.state_dict().keys() == {"proj.0.weight", "proj.0.bias"}


def test_mean_normal_over_mask():
    """The device sums in double and rounds the unit vector to fp32 once (2^-24); the reference sums 197 pixels in fp32 and its recorded
    vector is 6.6e-8 from the float64 value of the same pixels (computed on the CPU from the fixture's own map and mask): 2^-22 covers the
    two with a factor below 2 to spare."""
    got = frontend.mean_normal_over_mask(G["mean_normal_map"], G["mean_normal_mask"])
    assert tuple(got.shape) == (1, 3) and got.dtype == torch.float32 and got.is_cuda
    report("mean normal", got, G["mean_normal"], atol=2.0 ** -22)
    assert abs(float(got.norm()) - 1.0) < 1e-6
    with pytest.raises(ValueError):
        frontend.mean_normal_over_mask(G["mean_normal_map"], G["mean_normal_mask"][:, :5])


# ---- one layer on the reference's processor ABI -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("num_tokens", [1, 4])
def test_ip_processor_on_the_reference_operator_abi(num_tokens, dtype, tol):
    """MfhipIPAttnProcessor called the way Attention.forward calls its processor, on a stand-in with the reference layer's weights, against
    what the reference's Attention + IPAttnProcessor2_0(scale 0.7, num_tokens) returned (tolerances of tests/test_ops_gpu.py's plain twin)."""
    p = f"layer{num_tokens}_"
    w = lambda k: torch.from_numpy(G[p + k])

    class Attn(torch.nn.Module):                       # the attributes a processor reads (attention_processor.py:80-215)
        def __init__(self):
            super().__init__()
            self.heads, self.spatial_norm, self.group_norm, self.norm_cross = 8, None, None, None
            self.residual_connection, self.rescale_output_factor = False, 1.0
            self.to_q, self.to_k, self.to_v = (torch.nn.Linear(i, 64, bias=False) for i in (64, 32, 32))
            self.to_out = torch.nn.ModuleList([torch.nn.Linear(64, 64), torch.nn.Dropout(0.0)])

    attn = Attn()
    attn.load_state_dict({k: w(k) for k in ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_out.0.bias")})
    proc = MfhipIPAttnProcessor(64, 32, scale=0.7, num_tokens=num_tokens)
    proc.load_state_dict({"to_k_ip.weight": w("to_k_ip.weight"), "to_v_ip.weight": w("to_v_ip.weight")})
    attn, proc = attn.to(DEV, dtype), proc.to(DEV, dtype)
    with torch.no_grad():
        got = proc(attn, w("hidden_states").to(DEV, dtype), encoder_hidden_states=w("encoder_hidden_states").to(DEV, dtype))
    report(f"ip processor[{dtype}, num_tokens {num_tokens}]", got, G[p + "out"], atol=tol, rtol=tol)
    with pytest.raises(NotImplementedError):
        proc(attn, w("hidden_states").to(DEV, dtype), encoder_hidden_states=w("encoder_hidden_states").to(DEV, dtype),
             attention_mask=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):
        proc(attn, w("hidden_states").to(DEV, dtype))


# ---- UNet and pipeline ------------------------------------------------------------------------------------------------------------

def unet_inputs():
    g = torch.Generator().manual_seed(43)
    return torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 78, 32, generator=g)


@pytest.mark.parametrize("prec", PRECS)
def test_tiny_unet_with_ip_processors(prec):
    unet = build(prec)[0]
    x, ehs = unet_inputs()
    for t in (501, 21):
        eps = unet(x.to(DEV), t, ehs.to(DEV), return_dict=False)[0]
        check_ip(f"unet eps t={t}[{prec}]", eps, G[f"unet_eps_t{t}"], prec, TOL_UNET, f"ip_tiny/unet_eps_t{t}")
    # the ip branch is live: without the processors the same input gives another answer
    plain = M.UNet2DConditionModel(dict(TINY_UNET), precision=prec, device=DEV)
    plain.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    other = plain(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0]
    assert float((other.float().cpu() - torch.from_numpy(G["unet_eps_t501"])).abs().max()) > 1e-2


@pytest.mark.parametrize("prec", PRECS)
def test_tiny_pipeline_against_the_reference_wiring(prec):
    """4 DDIM steps, CFG 7.5, the normal given as a [1, 1, 3] vector through pipe.normal_embedder: per-step latents; the graph path and
    the eager path give the same bits; the token passed as ip_adapter_image_embeds (what get_normal_embeds returns) gives them too."""
    pipe = pipeline(prec)
    normal = torch.from_numpy(G["normals3"][1:2])
    trace = []
    run(pipe, normal, trace=trace)
    assert len(trace) == 4
    for i, l in enumerate(trace):
        check_ip(f"ip pipeline latents step {i}[{prec}]", l, G[f"pipeline_latents_{i}"], prec, TOL_PIPE, f"ip_tiny/pipeline_latents_{i}")
    pipe._graph_state = None
    graph = run(pipe, normal)
    pipe.use_hip_graph = False
    eager = run(pipe, normal)
    assert torch.equal(graph, eager), f"graph and eager latents differ by {float((graph - eager).abs().max())}"
    tok = pipe.normal_embedder(normal)
    assert torch.equal(run(pipe, embeds=[torch.cat([tok, tok])]), eager)
    assert torch.equal(run(pipe, embeds=[tok]), eager)


def test_pndm_graph_matches_eager():
    pipe = pipeline("f16x3", "pndm")
    normal = torch.from_numpy(G["normals3"][0:1])
    a = run(pipe, normal, steps=5)
    pipe.use_hip_graph = False
    b = run(pipe, normal, steps=5)
    assert torch.equal(a, b)


def test_new_normal_under_a_captured_graph():
    """Two calls with different normals and the same shapes: the second replays the first call's graph after bind_prompt refreshed K / V^T
    of the text AND of the ip tokens in place; it must equal a fresh pipeline's result bitwise."""
    pipe = pipeline("bf16")
    n0, n1 = torch.from_numpy(G["normals3"][0:1]), torch.from_numpy(G["normals3"][2:3])
    first = run(pipe, n0)
    assert pipe._graph_state is not None and pipe._graph_state["graph"] is not None
    graph = pipe._graph_state["graph"]
    second = run(pipe, n1, seed=99)
    assert pipe._graph_state["graph"] is graph, "the second call captured a new graph"
    _cache.pop("bf16")
    fresh = run(pipeline("bf16"), n1, seed=99)
    assert torch.equal(second, fresh), f"replayed and fresh latents differ by {float((second - fresh).abs().max())}"
    assert not torch.equal(first, second)


def test_checkpoint_round_trip_on_the_device(tmp_path):
    unet = build("fp32")[0]
    ck = checkpoint()
    back = unet.ip_adapter_state_dict()
    assert list(back) == list(ck["ip_adapter"]) and all(torch.equal(back[k].cpu(), ck["ip_adapter"][k]) for k in back)
    path = str(tmp_path / "ip-adapter.bin")
    torch.save({"image_proj": ck["image_proj"], "ip_adapter": back}, path)
    other = M.UNet2DConditionModel(dict(TINY_UNET), precision="fp32", device=DEV)
    other.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    proj = other.load_ip_adapter(path)
    assert all(torch.equal(proj[k], ck["image_proj"][k]) for k in proj)
    x, ehs = unet_inputs()
    assert torch.equal(other(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0], unet(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0])


def test_refusals(tmp_path):
    shapes = keys("tiny")
    cross = TINY_UNET["cross_attention_dim"]
    # training mode
    unet = M.UNet2DConditionModel(dict(TINY_UNET), precision="fp32", device=DEV)
    unet.load_state_dict(synth.state_dict_for(shapes["unet"], 0))
    unet.load_ip_adapter(checkpoint())
    with pytest.raises(NotImplementedError, match="inference only"):
        unet.train()
    trn = M.UNet2DConditionModel(dict(TINY_UNET), precision="fp32", device=DEV)
    trn.load_state_dict(synth.state_dict_for(shapes["unet"], 0))
    trn.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        trn.load_ip_adapter(checkpoint())
    # the XL UNet
    xl = M.UNet2DConditionModel(dict(TINY_XL_UNET), precision="fp32", device=DEV)
    xl.load_state_dict(synth.state_dict_for(keys("tiny_xl")["unet"], 0))
    with pytest.raises(NotImplementedError, match="SD1.5"):
        xl.set_attn_processor({n: MfhipAttnProcessor() if ".attn1." in n else MfhipIPAttnProcessor(xl.P[n[: -len("processor")] + "to_q"].n, 48)
                               for n in xl.attn_processors})
    # the mode without processors on the UNet
    pipe = pipeline("fp32")
    plain = M.UNet2DConditionModel(dict(TINY_UNET), precision="fp32", device=DEV)
    plain.load_state_dict(synth.state_dict_for(shapes["unet"], 0))
    pipe.unet = plain
    with pytest.raises(ValueError, match="IP-Adapter processors"):
        run(pipe, torch.from_numpy(G["normals3"][0:1]))
    # inputs of the other IP-Adapter kinds
    pipe = pipeline("fp32")
    with pytest.raises(NotImplementedError):
        pipe(prompt_embeds=torch.zeros(1, 77, cross), image=torch.zeros(1, 3, 16, 16), mask=torch.zeros(1, 3, 16, 16), ip_adapter_image=object())
    with pytest.raises(ValueError, match="normal_embedder"):
        pipe.normal_embedder = None
        run(pipe, torch.from_numpy(G["normals3"][0:1]))
    pipe.normal_embedder = build("fp32")[3]
    # a step program cannot hold the new entries
    with pytest.raises(program.ProgramError, match="has no replay thunk"):
        inp = synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=32, vae_scale=2)
        pipe.export_denoise_step(str(tmp_path / "step.mfprog"), prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                                 image=inp["image"], mask=inp["mask"], depth=inp["depth"], normals=torch.from_numpy(G["normals3"][0:1]),
                                 num_inference_steps=4, latents=inp["latents"].clone(), height=16, width=16)
    # the map-valued transform keeps refusing the mode and names the new function
    with pytest.raises(NotImplementedError, match="mean_normal_over_mask"):
        frontend.apply_transforms_normals(G["mean_normal_map"], 16, normals_conditioning_mode="ip_adapter")


# ---- the state the processors live in ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_processors_installed_on_the_cpu_follow_the_model_to_the_device(prec):
    """load_ip_adapter on a CPU-built UNet, then .to('cuda'): the ip branch runs on the device (fixture (c)), it is not dropped."""
    unet = M.UNet2DConditionModel(dict(TINY_UNET), precision=prec, device="cpu")
    unet.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    unet.load_ip_adapter(checkpoint())
    unet.to(DEV)
    x, ehs = unet_inputs()
    eps = unet(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0]
    check_ip(f"unet eps after .to(cuda)[{prec}]", eps, G["unet_eps_t501"], prec, TOL_UNET, "ip_tiny/unet_eps_t501")
    assert torch.equal(eps, build(prec)[0](x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0])
    # a layer that lost its processor is an error, not a plain attention over 78 tokens
    name = next(n for n in unet._ip_procs)
    unet._ip_procs.pop(name)
    unet._cross_kv = {}
    with pytest.raises(RuntimeError, match="would be dropped"):
        unet(x.to(DEV), 501, ehs.to(DEV), return_dict=False)


def test_scale_is_read_from_the_live_processor():
    """The reference's set_scale idiom, proc.scale = s on the objects attn_processors hands back: the next forward uses it, and a
    pipeline call after it does not replay a graph captured with the old scale."""
    unet = M.UNet2DConditionModel(dict(TINY_UNET), precision="f16x3", device=DEV)
    unet.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    unet.load_ip_adapter(checkpoint())
    x, ehs = unet_inputs()
    one = unet(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0].clone()
    report("scale 1.0", one, G["unet_eps_t501"], **TOL_UNET)
    sig = unet.ip_signature()
    for p in unet.attn_processors.values():
        if isinstance(p, MfhipIPAttnProcessor):
            p.scale = 0.25
    assert unet.ip_signature() != sig
    quarter = unet(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0].clone()
    assert float((quarter - one).abs().max()) > 1e-2
    other = M.UNet2DConditionModel(dict(TINY_UNET), precision="f16x3", device=DEV)
    other.load_state_dict(synth.state_dict_for(keys("tiny")["unet"], 0))
    other.load_ip_adapter(checkpoint(), scale=0.25)
    assert torch.equal(quarter, other(x.to(DEV), 501, ehs.to(DEV), return_dict=False)[0])


def test_two_prompts_two_images_each_pair_tokens_with_their_prompts():
    """B = 2 prompts with different normals, num_images_per_prompt = 2, under CFG: image j (prompt j // 2) must equal the B = 1 run of
    prompt j // 2 with that image's latents and conditioning noise (another batch size picks other GEMM tiles: the pipeline's 1e-3, as
    tests/test_pipeline_gpu.py's shard test), and must NOT equal the run with the other prompt's normal."""
    pipe = pipeline("fp32")
    g = torch.Generator().manual_seed(5)
    a, b = synth.pipeline_inputs(1, 16, 16, seed=11, cross_dim=32, vae_scale=2), synth.pipeline_inputs(1, 16, 16, seed=12, cross_dim=32, vae_scale=2)
    cat = lambda k: torch.cat([a[k], b[k]])
    latents, noise = torch.randn(4, 4, 8, 8, generator=g), torch.randn(8, 4, 8, 8, generator=g)
    normals = torch.from_numpy(G["normals3"][[0, 2]])                       # [2, 1, 3]
    common = dict(num_inference_steps=4, guidance_scale=7.5, output_type="latent", height=16, width=16)
    full = pipe(prompt_embeds=cat("prompt_embeds"), negative_prompt_embeds=cat("negative_prompt_embeds"), image=cat("image"), mask=cat("mask"),
                depth=cat("depth"), normals=normals, num_images_per_prompt=2, latents=latents.clone(), conditioning_noise=noise,
                **common).images.float().cpu()
    tok = pipe.normal_embedder(normals)
    stacked = pipe(prompt_embeds=cat("prompt_embeds"), negative_prompt_embeds=cat("negative_prompt_embeds"), image=cat("image"), mask=cat("mask"),
                   depth=cat("depth"), ip_adapter_image_embeds=[torch.cat([tok, tok])], num_images_per_prompt=2, latents=latents.clone(),
                   conditioning_noise=noise, **common).images.float().cpu()
    assert torch.equal(full, stacked)

    def single(j, which_normal):
        src = (a, b)[j // 2]
        return pipe(prompt_embeds=src["prompt_embeds"], negative_prompt_embeds=src["negative_prompt_embeds"], image=src["image"], mask=src["mask"],
                    depth=src["depth"], normals=normals[which_normal:which_normal + 1], latents=latents[j:j + 1].clone(),
                    conditioning_noise=torch.cat([noise[j:j + 1], noise[4 + j:5 + j]]), **common).images.float().cpu()
    for j in range(4):
        report(f"image {j} of the 2 x 2 batch vs its own B = 1 run", full[j:j + 1], single(j, j // 2), **TOL_PIPE)
        assert float((full[j:j + 1] - single(j, 1 - j // 2)).abs().max()) > 10 * TOL_PIPE["atol"], "the other prompt's normal gives the same image"
    with pytest.raises(ValueError, match="one token per prompt"):
        pipe(prompt_embeds=cat("prompt_embeds"), negative_prompt_embeds=cat("negative_prompt_embeds"), image=cat("image"), mask=cat("mask"),
             depth=cat("depth"), ip_adapter_image_embeds=[tok[:1].repeat(3, 1, 1)], num_images_per_prompt=2, latents=latents.clone(),
             conditioning_noise=noise, **common)
