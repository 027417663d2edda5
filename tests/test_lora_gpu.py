"""LoRA adapters on the GPU: mf_lora_merge against float64 per element, the tiny UNets against the reference's recorded outputs
(tests/golden/lora_tiny.npz, tools/make_golden_lora.py) in every precision, and the properties of the always-merged design: the
selective rebuild equals a full one bit for bit, un-merging is exact, a scale round trip returns the same bits."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_ref  # noqa: E402
from oracle import mirrorfusion_ref as R  # noqa: E402
from reflecting_reality_amd import DDIMScheduler, StableDiffusionBrushNetPipeline, configs, hip, lora, models as M, synth  # noqa: E402
from reflecting_reality_amd.ops import ConvWeight  # noqa: E402
from reflecting_reality_amd.text_encoder import CLIPTextModel  # noqa: E402
from test_lora_cpu import fixture_inputs  # noqa: E402
from test_models_gpu import PRECS, TOL, build  # noqa: E402
from util import ENV_K_LINF, ENV_K_LINF_SMALL, ENV_K_MEAN, ENV_SMALL_NUMEL, GOLD, golden, keys, report  # noqa: E402

DEV = "cuda"
F32TOL = dict(atol=2e-4, rtol=2e-4)
CASES = {"tiny": (R.TINY_UNET, 0), "tiny_xl": (R.TINY_XL_UNET, 20)}
_ref = {}


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
# (rows, cols, ranks): a wide row block, conv_in's cols = 36, odd sizes (scalar accesses), two terms, the largest SD1.5 Linear at rank
# 128 (two row-tile columns, eight rank chunks), and a single element
KERNEL_TARGETS = [(4, 2880, (4,)), (320, 36, (8,)), (33, 65, (3,)), (64, 288, (16, 5)), (1280, 1280, (128,)), (1, 1, (1,))]


def kernel_case():
    """The inputs, the float64 result and its bound, computed once and left unchanged."""
    if "kernel" not in _ref:
        g = torch.Generator().manual_seed(11)
        tg = []
        for rows, cols, ranks in KERNEL_TARGETS:
            base = torch.randn(rows, cols, generator=g)
            terms = [(torch.randn(rows, r, generator=g), torch.randn(r, cols, generator=g) / r ** 0.5,
                      float(torch.randn((), generator=g)) * 0.5) for r in ranks]
            ref, mag = lora_ref.merge64(base, terms)
            tg.append((base, terms, ref, lora_ref.bound(terms, mag)))
        _ref["kernel"] = tg
    return _ref["kernel"]


def launch(case, coefs=None):
    targets, outs, cf = [], [], []
    for base, terms, _, _ in case:
        out = torch.full(base.shape, float("nan"), device=DEV)
        targets.append((base.to(DEV), out, [(up.to(DEV), down.to(DEV)) for up, down, _ in terms]))
        outs.append(out)
        cf += [c for _, _, c in terms]
    tables = hip.LoraTables(targets, DEV)
    hip.lora_merge(tables, cf if coefs is None else coefs)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], tables


def test_kernel_against_float64_per_element_in_one_grouped_launch():
    case = kernel_case()
    outs, tables = launch(case)
    assert tables.ntargets == len(KERNEL_TARGETS) and tables.nterms == sum(len(r) for _, _, r in KERNEL_TARGETS)
    for (rows, cols, ranks), (base, terms, ref, bnd), out in zip(KERNEL_TARGETS, case, outs):
        err = (out.double() - ref).abs()
        worst = float((err / bnd).max())
        print(f"lora_merge {rows} x {cols} ranks {ranks}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
        assert torch.isfinite(out).all()
        assert bool((err <= bnd).all()), f"{rows} x {cols}: {int((err > bnd).sum())} elements over the bound, worst ratio {worst:.3f}"
    again, _ = launch(case)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "two runs differ"
    zero, _ = launch(case, [0.0] * tables.nterms)
    assert all(torch.equal(z, base) for z, (base, _, _, _) in zip(zero, case)), "coef 0 must leave the base bit for bit"


def test_wrapper_refuses_what_the_entry_refuses():
    base = torch.zeros(4, 8, device=DEV)
    up, down = torch.zeros(4, 2, device=DEV), torch.zeros(2, 8, device=DEV)
    with pytest.raises(hip.MfhipError, match="must not alias"):
        hip.lora_merge(hip.LoraTables([(base, base, [(up, down)])], DEV), [1.0])
    with pytest.raises(hip.MfhipError, match="do not fit"):
        hip.LoraTables([(base, torch.zeros_like(base), [(up, torch.zeros(3, 8, device=DEV))])], DEV)


# ---- the tiny UNets against the reference ------------------------------------------------------------------------------------------------
def fresh_unet(case, prec, sd=None):
    cfg, wseed = CASES[case]
    unet = M.UNet2DConditionModel(dict(cfg), precision=prec, device=DEV)
    unet.load_state_dict(sd if sd is not None else synth.state_dict_for(keys(case)["unet"], wseed))
    return unet


def run(unet, G, case, **kw):
    x, ehs, added, t = fixture_inputs(G, case)
    if added:
        kw["added_cond_kwargs"] = {k: v.to(DEV) for k, v in added.items()}
    return unet(x.to(DEV), t, ehs.to(DEV), return_dict=False, **kw)[0].float().cpu()


def check_fixture(name, got, ref, prec, case, key):
    if prec in ("fp32", "f16x3"):
        return report(name, got, ref, **TOL[prec])
    if "env" not in _ref:
        with open(os.path.join(GOLD, "lora_envelope.json")) as f:
            _ref["env"] = json.load(f)
    env = _ref["env"][f"{prec}/{case}/{key}"]
    err = (got - torch.as_tensor(ref)).abs()
    k_linf = ENV_K_LINF if err.numel() >= ENV_SMALL_NUMEL else ENV_K_LINF_SMALL
    linf, mean = float(err.max()), float(err.mean())
    print(f"{name}: max_abs_err={linf:.3e} (reference {prec}: {env['linf']:.3e}) mean_abs_err={mean:.3e} (reference {prec}: {env['mean']:.3e}) "
          f"ENVRATIO linf {linf / env['linf']:.3f} mean {mean / env['mean']:.3f}")
    assert linf == linf and linf <= k_linf * env["linf"], f"{name}: L-inf {linf:.3e} > {k_linf} x the reference's {prec} envelope {env['linf']:.3e}"
    assert mean <= ENV_K_MEAN * env["mean"], f"{name}: mean error {mean:.3e} > {ENV_K_MEAN} x the reference's {prec} envelope {env['mean']:.3e}"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("prec", PRECS)
def test_tiny_unets_match_the_reference_unfused_fused_and_at_scale_one(case, prec):
    G = golden("lora_tiny.npz")
    unet = fresh_unet(case, prec)
    asd, alphas = lora_ref.adapter_of(G, case, unet.param_shapes(), prefix="unet.")
    check_fixture(f"{case} base[{prec}]", run(unet, G, case), G[f"{case}_base"], prec, case, "base")
    unet.load_attn_procs(asd, network_alphas=alphas)
    check_fixture(f"{case} scale 0.7[{prec}]", run(unet, G, case, cross_attention_kwargs={"scale": 0.7}), G[f"{case}_s07"], prec, case, "s07")
    check_fixture(f"{case} scale 1.0[{prec}]", run(unet, G, case), G[f"{case}_s10"], prec, case, "s10")
    unet.fuse_lora(0.7)
    fused = run(unet, G, case, cross_attention_kwargs={"scale": 0.2})            # pinned: the call's scale has no effect
    check_fixture(f"{case} fused 0.7[{prec}]", fused, G[f"{case}_fused07"], prec, case, "fused07")
    with pytest.raises(NotImplementedError, match="only 'scale'"):
        run(unet, G, case, cross_attention_kwargs={"scale": 0.7, "gligen": {}})


def test_fp8_is_finite_and_equals_its_own_build_from_the_merged_weights():
    G = golden("lora_tiny.npz")
    unet = fresh_unet("tiny_xl", "fp8")
    asd, alphas = lora_ref.adapter_of(G, "tiny_xl", unet.param_shapes())
    unet.load_attn_procs(asd, network_alphas=alphas)
    unet.fuse_lora(0.7)
    got = run(unet, G, "tiny_xl")
    assert torch.isfinite(got).all()
    assert float((got - torch.from_numpy(G["tiny_xl_base"])).abs().max()) >= 0.05
    assert torch.equal(got, run(fresh_unet("tiny_xl", "fp8", unet.state_dict()), G, "tiny_xl"))


# ---- the selective rebuild is a full rebuild -------------------------------------------------------------------------------------------------
WIDE = dict(in_channels=4, out_channels=4, block_out_channels=(320,), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D",),
            up_block_types=("CrossAttnUpBlock2D",), cross_attention_dim=64, attention_head_dim=8, norm_num_groups=32)


def wide_unet(prec, sd=None):
    unet = M.UNet2DConditionModel(dict(WIDE), precision=prec, device=DEV)
    unet.load_state_dict(sd if sd is not None else synth.state_dict_for(unet.param_shapes(), 5))
    return unet


def wide_run(unet, **kw):
    g = torch.Generator().manual_seed(3)
    x, ehs = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 77, 64, generator=g)
    return unet(x.to(DEV), 301, ehs.to(DEV), return_dict=False, **kw)[0].float().cpu()


@pytest.mark.parametrize("prec", ["bf16", "f16x3"])
def test_a_fresh_model_from_the_fused_state_dict_gives_the_same_bits(prec):
    """Width 320 reaches the LayerNorm folds, q | k | v and both GEGLU forms in bf16: every derived layout of a targeted weight."""
    unet = wide_unet(prec)
    base = wide_run(unet)
    if prec == "bf16":
        assert any(k.endswith("to_qkv_ln") for k in unet.P) and any(k.endswith("proj_ln") for k in unet.P)
    asd, alphas = synth.lora_adapter(synth.lora_plan(unet.lora_modules()), unet.param_shapes(), 7, 0.3, prefix="")
    unet.load_attn_procs(asd, network_alphas=alphas)
    unet.fuse_lora(0.7)
    wide_run(unet)                                       # (the first pass picks the GEMM tiles both models then share)
    fused = wide_run(unet)
    assert float((fused - base).abs().max()) >= 0.05
    sd = unet.state_dict()
    assert not torch.equal(sd["conv_in.weight"], unet._src["conv_in.weight"])          # the merged weights, as the reference saves them
    assert torch.equal(wide_run(wide_unet(prec, sd)), fused)
    unet.unfuse_lora()
    assert torch.equal(unet.state_dict()["conv_in.weight"], unet._src["conv_in.weight"])


# ---- restore, scale changes, several adapters -----------------------------------------------------------------------------------------------
def device_weights(unet):
    out = {k: v.w for k, v in unet.P.items() if isinstance(v, ConvWeight)}
    out.update({k: getattr(unet, k).w for k in ("te1", "te2", "temb_proj")})
    return out


def test_unfuse_and_unload_restore_the_base_bit_for_bit():
    G = golden("lora_tiny.npz")
    plain, unet = fresh_unet("tiny", "bf16"), fresh_unet("tiny", "bf16")
    base = run(plain, G, "tiny")
    asd, alphas = lora_ref.adapter_of(G, "tiny", unet.param_shapes())
    unet.load_attn_procs(asd, network_alphas=alphas)
    s10 = run(unet, G, "tiny")
    unet.fuse_lora(0.7)
    assert not torch.equal(run(unet, G, "tiny"), base)
    unet.unfuse_lora()                                   # the device weights are the base again ...
    want = device_weights(plain)
    assert all(torch.equal(w, want[k]) for k, w in device_weights(unet).items())
    assert torch.equal(run(unet, G, "tiny"), s10)        # ... and the adapter is active again at scale 1.0, as the reference's unfused layers
    assert torch.equal(run(unet, G, "tiny", cross_attention_kwargs={"scale": 0.0}), base)
    unet.unload_lora()
    assert unet._lora_state() is None and torch.equal(run(unet, G, "tiny"), base)
    with pytest.raises(NotImplementedError, match="LoRA-scale"):                       # no adapter: today's refusal, word for word
        run(unet, G, "tiny", cross_attention_kwargs={"scale": 0.5})


def test_only_the_targeted_entries_are_rebuilt():
    unet = fresh_unet("tiny", "bf16")
    k = "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k"
    before, temb = dict(unet.P), unet.temb_proj
    asd, _ = synth.lora_adapter([(k, 4, 2.0)], unet.param_shapes(), 7, 0.5, prefix="")
    unet.load_attn_procs(asd)
    unet._lora_sync()
    assert set(unet.P) == set(before) and unet.temb_proj is temb
    assert [n for n in before if unet.P[n] is not before[n]] == [k]
    unet.unload_lora()
    assert [n for n in before if unet.P[n] is not before[n]] == [k]


def test_scale_round_trip_returns_the_same_bits():
    G = golden("lora_tiny.npz")
    unet = fresh_unet("tiny", "fp32")
    asd, alphas = lora_ref.adapter_of(G, "tiny", unet.param_shapes())
    unet.load_attn_procs(asd, network_alphas=alphas)
    gen = unet._weights_gen
    first = run(unet, G, "tiny", cross_attention_kwargs={"scale": 0.7})
    assert unet._weights_gen == gen + 1
    assert torch.equal(run(unet, G, "tiny", cross_attention_kwargs={"scale": 0.7}), first) and unet._weights_gen == gen + 1     # no re-merge
    assert not torch.equal(run(unet, G, "tiny", cross_attention_kwargs={"scale": 0.3}), first)
    assert torch.equal(run(unet, G, "tiny", cross_attention_kwargs={"scale": 0.7}), first) and unet._weights_gen == gen + 3


def test_set_adapters_is_the_weighted_sum_of_the_host_merged_build():
    G = golden("lora_tiny.npz")
    unet = fresh_unet("tiny", "fp32")
    shapes, mods = unet.param_shapes(), unet.lora_modules()
    a = synth.lora_adapter(synth.lora_plan(mods[::2]), shapes, 31, 0.5, prefix="unet.")
    b = synth.lora_adapter(synth.lora_plan(mods[1::3]), shapes, 32, 0.5, prefix="")            # overlaps a on some targets: two terms there
    unet.load_attn_procs(a[0], network_alphas=a[1], adapter_name="a")
    unet.load_attn_procs(b[0], network_alphas=b[1], adapter_name="b")
    with pytest.raises(ValueError, match="already loaded"):
        unet.load_attn_procs(b[0], adapter_name="b")
    with pytest.raises(ValueError, match="'c'"):
        unet.set_adapters(["a", "c"])
    unet.set_adapters(["a", "b"], [0.7, 0.3])
    assert unet.active_adapters() == ["a", "b"]
    got = run(unet, G, "tiny")
    merged = lora_ref.host_merged(unet._src, shapes, mods, [(a[0], a[1], 0.7), (b[0], b[1], 0.3)])
    report("set_adapters vs host-merged build", got, run(fresh_unet("tiny", "fp32", merged), G, "tiny"), **F32TOL)
    assert float((got - torch.from_numpy(G["tiny_base"])).abs().max()) >= 0.05
    unet.set_adapters("b")
    only_b = lora_ref.host_merged(unet._src, shapes, mods, [(b[0], b[1], 1.0)])
    report("set_adapters('b') vs host-merged build", run(unet, G, "tiny"), run(fresh_unet("tiny", "fp32", only_b), G, "tiny"), **F32TOL)


def test_safe_fusing_refuses_non_finite_weights_and_changes_nothing():
    G = golden("lora_tiny.npz")
    unet = fresh_unet("tiny", "fp32")
    k = "mid_block.resnets.0.conv1"
    asd, _ = synth.lora_adapter([(k, 4, None)], unet.param_shapes(), 7, 0.5, prefix="")
    asd[k + ".lora.up.weight"][0, 0] = float("inf")
    unet.load_attn_procs(asd)
    before = dict(unet.P)
    with pytest.raises(ValueError, match="not finite"):
        unet.fuse_lora(1.0, safe_fusing=True)
    assert all(unet.P[n] is before[n] for n in before) and unet._lora_state().pinned is None
    unet.unload_lora()
    assert torch.isfinite(run(unet, G, "tiny")).all()


# ---- pipeline, text encoder, refusals -----------------------------------------------------------------------------------------------------
def tiny_pipe(unet, prec):
    _, bn, vae = build("tiny", prec)
    sched = DDIMScheduler(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                          set_alpha_to_one=False, clip_sample=False)
    pipe = StableDiffusionBrushNetPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=unet, brushnet=bn, scheduler=sched,
                                           safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           depth_conditioning_mode="concat")
    pipe.set_progress_bar_config(disable=True)
    return pipe


def pipe_run(pipe, **kw):
    inp = synth.pipeline_inputs(1, 16, 16, seed=1234, cross_dim=32, vae_scale=2)
    noise = torch.from_numpy(golden("tiny_pipeline.npz")["ddim_vae_noise"])
    return pipe(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"], image=inp["image"],
                mask=inp["mask"], depth=inp["depth"], num_inference_steps=4, guidance_scale=7.5, latents=inp["latents"].clone(),
                output_type="latent", height=16, width=16, conditioning_noise=noise, **kw).images.float().cpu()


def test_pipeline_with_the_captured_step_graph(tmp_path):
    G = golden("lora_tiny.npz")
    pipe = tiny_pipe(fresh_unet("tiny", "bf16"), "bf16")
    assert pipe.use_hip_graph
    with pytest.raises(NotImplementedError, match="are not built"):                    # no adapter: today's refusal
        pipe_run(pipe, cross_attention_kwargs={"scale": 0.5})
    first = pipe_run(pipe)
    asd, alphas = lora_ref.adapter_of(G, "tiny", pipe.unet.param_shapes(), prefix="unet.")
    pipe.load_lora_weights({**asd, **{k: torch.tensor(v) for k, v in alphas.items()}}, adapter_name="style")
    assert pipe.get_active_adapters() == ["style"]
    loaded = pipe_run(pipe)
    assert not torch.equal(loaded, first) and float((loaded - first).abs().max()) > 0.05
    assert not torch.equal(pipe_run(pipe, cross_attention_kwargs={"scale": 0.5}), loaded)
    with pytest.raises(NotImplementedError, match="fuse_lora"):
        pipe.export_call(str(tmp_path), prompt="a mirror")
    pipe.fuse_lora(lora_scale=0.7)
    fused = pipe_run(pipe)
    other = tiny_pipe(fresh_unet("tiny", "bf16", pipe.unet.state_dict()), "bf16")
    assert torch.equal(pipe_run(other), fused)
    pipe.unload_lora_weights()
    assert pipe.get_active_adapters() == [] and torch.equal(pipe_run(pipe), first)


def test_text_encoder_takes_kohya_keys():
    cfg = configs.TINY_CLIP_L_TEXT
    shapes = CLIPTextModel(dict(cfg), precision="fp32", device="cpu").param_shapes()
    sd = synth.state_dict_for(shapes, 3)
    te = CLIPTextModel(dict(cfg), precision="fp32", device=DEV)
    te.load_state_dict(sd)
    mods = te.lora_modules()
    assert len(mods) == 6 * cfg["num_hidden_layers"]
    dotted, alphas = synth.lora_adapter(synth.lora_plan(mods), shapes, 9, 0.5, prefix="text_encoder.")
    kohya = {}
    for m, r, a in synth.lora_plan(mods):
        k = "lora_te_" + m.replace(".", "_")
        kohya[k + ".lora_down.weight"] = dotted[f"text_encoder.{m}.lora.down.weight"]
        kohya[k + ".lora_up.weight"] = dotted[f"text_encoder.{m}.lora.up.weight"]
        if a is not None:
            kohya[k + ".alpha"] = torch.tensor(a)
    ids = torch.randint(0, cfg["vocab_size"] - 1, (2, 77), generator=torch.Generator().manual_seed(1))
    ids[:, -1] = cfg["vocab_size"] - 1
    base = te(ids)[0].cpu()
    te.load_lora(kohya)
    got = te(ids)[0].cpu()
    ref = CLIPTextModel(dict(cfg), precision="fp32", device=DEV)
    ref.load_state_dict(lora_ref.host_merged(sd, shapes, mods, [(dotted, alphas, 1.0)]))
    report("text encoder, kohya adapter vs host-merged build", got, ref(ids)[0].cpu(), **F32TOL)
    assert float((got - base).abs().max()) >= 0.05
    te.unload_lora()
    assert torch.equal(te(ids)[0].cpu(), base)


def test_refusals():
    unet = fresh_unet("tiny", "fp32")
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    asd, _ = synth.lora_adapter([(q, 4, None)], unet.param_shapes(), 7, 0.5, prefix="")
    _, bn, _ = build("tiny", "fp32")
    with pytest.raises(NotImplementedError, match="BrushNet"):
        bn.load_attn_procs(asd)
    unet.load_attn_procs(asd)
    for go in (unet.train, unet.prepare_training):
        with pytest.raises(NotImplementedError, match="LoRA"):
            go()
    with pytest.raises(RuntimeError, match="unload_lora"):
        unet.load_state_dict(unet._src)
    unet.unload_lora()
    unet.prepare_training(requires_grad=False)
    with pytest.raises(NotImplementedError, match="training layout"):
        unet.load_attn_procs(asd)
    from reflecting_reality_amd import StableDiffusionXLBrushNetPipeline as XL
    xl = XL.__new__(XL)
    with pytest.raises(NotImplementedError, match="SD1.5 pipeline"):
        xl.load_lora_weights(asd)
    with pytest.raises(NotImplementedError, match="SD1.5 pipeline"):
        xl.fuse_lora()
