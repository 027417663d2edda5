"""Model / scheduler configurations of the BASELINE workloads (the subset of config.json the hot path reads).

SD1.5 values: runwayml/stable-diffusion-v1-5 `unet/config.json`, `vae/config.json`, `scheduler/scheduler_config.json`
(those files are external to the reference tree).  BrushNet: BrushNetModel.from_unet with
conditioning_channels = 6 (4 masked-image latents + mask + depth; examples/brushnet/train_brushnet_mirror.py:968-971).
"""
SD15_UNET = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    cross_attention_dim=768, attention_head_dim=8, norm_num_groups=32, norm_eps=1e-5,
    flip_sin_to_cos=True, freq_shift=0)
SD15_VAE = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512),
                layers_per_block=2, norm_num_groups=32, scaling_factor=0.18215)
SD15_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                  steps_offset=1, set_alpha_to_one=False, clip_sample=False, skip_prk_steps=True)

TINY_UNET = dict(
    in_channels=4, out_channels=4, block_out_channels=(32, 64), layers_per_block=2,
    down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
    cross_attention_dim=32, attention_head_dim=4, norm_num_groups=32, norm_eps=1e-5,
    flip_sin_to_cos=True, freq_shift=0)
TINY_VAE = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(32, 64), layers_per_block=1,
                norm_num_groups=32, scaling_factor=0.18215)

# SDXL (stabilityai/stable-diffusion-xl-base-1.0 unet/config.json) and a tiny configuration of the
# same architecture: linear proj_in/proj_out, per-level transformer depth and head count, text_time embedding
SDXL_UNET = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280), layers_per_block=2,
    down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
    up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
    cross_attention_dim=2048, attention_head_dim=(5, 10, 20), transformer_layers_per_block=(1, 2, 10),
    use_linear_projection=True, addition_embed_type="text_time", addition_time_embed_dim=256,
    projection_class_embeddings_input_dim=2816, norm_num_groups=32, norm_eps=1e-5, flip_sin_to_cos=True, freq_shift=0)
SDXL_VAE = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512),
                layers_per_block=2, norm_num_groups=32, scaling_factor=0.13025)
TINY_XL_UNET = dict(
    in_channels=4, out_channels=4, block_out_channels=(32, 64, 64), layers_per_block=2,
    down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
    up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
    cross_attention_dim=48, attention_head_dim=(2, 4, 8), transformer_layers_per_block=(1, 2, 3),
    use_linear_projection=True, addition_embed_type="text_time", addition_time_embed_dim=8,
    projection_class_embeddings_input_dim=6 * 8 + 24, norm_num_groups=32, norm_eps=1e-5, flip_sin_to_cos=True, freq_shift=0)


def brushnet_config(unet_cfg: dict, conditioning_channels: int = 6) -> dict:
    n = len(unet_cfg["block_out_channels"])
    cfg = dict(unet_cfg)
    cfg.pop("out_channels", None)
    cfg.update(conditioning_channels=conditioning_channels, down_block_types=("DownBlock2D",) * n,
               up_block_types=("UpBlock2D",) * n, mid_block_type="MidBlock2D")
    return cfg


# CLIP text encoders (transformers CLIPTextConfig fields; text_encoder.py).  CLIP_L_TEXT: openai/clip-vit-large-patch14 as shipped in
# SD1.5 / SDXL `text_encoder/config.json` (legacy eos_token_id 2: the pooled row is argmax(input_ids)); OPENCLIP_BIGG_TEXT: SDXL's
# `text_encoder_2` (OpenCLIP ViT-bigG/14, 32 layers, with text projection; padded with 0).  The tiny pair has the same two styles.
# tools/make_golden_clip.py, tools/bench_text_encoder.py and the tests all read these: one source.
CLIP_L_TEXT = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                   max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=768, eos_token_id=2)
OPENCLIP_BIGG_TEXT = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                          max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=1280, eos_token_id=49407)
TINY_CLIP_L_TEXT = dict(vocab_size=1000, hidden_size=32, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                        max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=16, eos_token_id=2)
TINY_CLIP_G_TEXT = dict(vocab_size=1000, hidden_size=32, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                        max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=16, eos_token_id=999)
# fixture name (tests/golden/clip_<name>.npz) -> (config, has a text projection).  bigg4: bigG at full width, cut to 4 layers so that
# the float64 run and the fixture stay small.
CLIP_FIXTURES = {
    "tiny_l": (TINY_CLIP_L_TEXT, False), "tiny_g": (TINY_CLIP_G_TEXT, True), "clip_l": (CLIP_L_TEXT, False),
    "bigg4": (dict(OPENCLIP_BIGG_TEXT, num_hidden_layers=4), True),
}
# CLIP vision towers (transformers CLIPVisionConfig fields; image_encoder.py).  CLIP_L_VISION: openai/clip-vit-large-patch14, the scorer of
# the reference's CLIP_Similarity (metrics/metrics.py:156-157) and the image encoder examples/brushnet/ip_adapter/ loads.  The tiny ones
# (tools/make_golden_clip_vision.py): tiny_vit_a 17 tokens, K = 192; tiny_vit_b K = 147 -> 152 (pad columns); vit_d64 ViT-L/14's patch
# width and head dim; vit_l4 ViT-L/14 at full width cut to 4 layers (257 tokens: one query row alone in the third q-tile).
CLIP_L_VISION = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
                     num_channels=3, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=768)
TINY_VIT_A = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, image_size=32, patch_size=8,
                  num_channels=3, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=16)
TINY_VIT_B = dict(TINY_VIT_A, image_size=28, patch_size=7)
VIT_D64 = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14,
               num_channels=3, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=32)
# fixture name (tests/golden/clip_<name>.npz) -> config; every one is a CLIPVisionModelWithProjection
CLIP_VISION_FIXTURES = {"tiny_vit_a": TINY_VIT_A, "tiny_vit_b": TINY_VIT_B, "vit_d64": VIT_D64,
                        "vit_l4": dict(CLIP_L_VISION, num_hidden_layers=4)}
# tiny_clip: a CLIPModel of tiny_l's text tower and tiny_vit_a, projection 16 (captions through synth.HashTokenizer)
TINY_CLIP = dict(projection_dim=16, logit_scale_init_value=2.6592, text_config=dict(TINY_CLIP_L_TEXT), vision_config=dict(TINY_VIT_A))
# openai/clip-vit-large-patch14 as a CLIPModel (tools/bench_clip_score.py)
CLIP_L = dict(projection_dim=768, logit_scale_init_value=2.6592, text_config=dict(CLIP_L_TEXT), vision_config=dict(CLIP_L_VISION))
