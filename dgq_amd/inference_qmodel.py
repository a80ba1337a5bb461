"""Drop-in counterpart of the reference CLI ``src/inference_qmodel.py`` (same flag names, :16-44).

The reference builds a diffusers pipeline from pretrained weights (src/utils.py:16-54: needs network + HF
checkpoints, out of scope) and renders PNGs.  No pretrained weights exist in this environment, so this CLI runs the
same quantized-UNet path — ``get_qmodel`` → ``half()/float()`` → ``disable_out_quantization()`` → denoise loop
(src/inference_qmodel.py:91-108) — on synthetic name-keyed weights and latents, and saves the final latents.
With ``--cali_ckpt`` pointing at a real merged checkpoint and ``--unet_weights`` at an HF UNet state-dict the very
same code path serves real weights.  It does not end in ``breakpoint()`` (:110).

Multi-GPU: run under ``python -m torch.distributed.run --nproc-per-node N``; every rank takes its slice of the
prompt list (src/gen4eval_SDXL.py:116), no collective on the data path.
"""
import argparse
import logging
import os
import types

import torch

from . import synth
from .runtime import denoise_loop, shard_prompts

MODEL_TYPE = os.environ.get("DIFFUSERS_REWRITE", "sd")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Quantized UNet inference (DGQ) on MI355X")
    p.add_argument("--use_group", action="store_true", help="Use group quantization")
    p.add_argument("--num_inference_steps", type=int, default=-1)
    p.add_argument("--prompt", type=str, default="a painting of a virus monster playing guitar")
    p.add_argument("--cali_ckpt", type=str, default=None, help="merged calibration checkpoint (synthetic if omitted)")
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--wq", type=int, default=4)
    p.add_argument("--use_aq", action="store_true")
    p.add_argument("--aq", type=int, default=8)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--t2i_log_quant", action="store_true")
    p.add_argument("--t2i_real_time", action="store_true")
    p.add_argument("--t2i_start_peak", action="store_true")
    p.add_argument("--time_aware_aqtizer", action="store_true")
    # additions (no counterpart in the reference)
    p.add_argument("--model_type", default=MODEL_TYPE, choices=["sd", "sdxl", "tiny", "mini"])
    p.add_argument("--unet_weights", default=None, help="HF-keyed UNet state-dict (.pt); synthetic if omitted")
    p.add_argument("--group_num", type=int, default=16, help="G of the synthetic checkpoint")
    p.add_argument("--n_prompts", type=int, default=2, help="synthetic prompts (the reference renders 2 images)")
    p.add_argument("--out", default="latents_{rank}.pt")
    p.add_argument("--graphs", action="store_true", help="replay one hipGraph per timestep slot")
    p.add_argument("--aq_real_time", action="store_true",
                   help="with --use_aq: per-row activation parameters taken from every call's own rows (Scaler.MINMAX per row, "
                        "dgq_act_row_params) — runs from a weight-only checkpoint, no activation calibration")
    p.add_argument("--aq_real_time_block", type=int, default=0,
                   help="with --aq_real_time: 32 = one pair per row and block of 32 consecutive channels (dgq_quant_act_block + "
                        "dgq_gemm_blockq); 0 = one pair per row")
    p.add_argument("--aq_real_time_format", default="int", choices=("int", "mxfp6"),
                   help="with --aq_real_time --aq_real_time_block 32 and 6 activation bits: mxfp6 = every block one power-of-two scale and "
                        "32 FP6 E2M3 codes on the block-scaled matrix cores (dgq_quant_act_mx6 + dgq_gemm_mx6; W4 layers, W4A6)")
    p.add_argument("--wq_mfma16", action="store_true",
                   help="weight-only state (no --use_aq): run the layers on the bf16 / f16 matrix cores (dgq_conv2d_wq_mfma16) — faster, "
                        "not bit-identical to the default exact route")
    p.add_argument("--wq_fused", action="store_true",
                   help="with --wq_mfma16: fold GroupNorm / LayerNorm, SiLU, GEGLU, residual adds and the time-embedding rows into the "
                        "layers' launches (dgq_conv2d_wq_mfma16_fused) instead of torch operators around them — differs by rounding")
    p.add_argument("--attn_mfma16", action="store_true",
                   help="with --fp16 and no --use_aq: run the un-quantised attentions on the f16 matrix cores in one launch "
                        "(dgq_attention_mfma16) instead of matmul / softmax / matmul — faster, differs by rounding")
    p.add_argument("--attn_mfma16_fp32", action="store_true",
                   help="fp32 state (no --fp16, no --use_aq): run the un-quantised attentions on the bf16 matrix cores in one launch "
                        "(dgq_attention_mfma16_f32, two-term bf16 splits) instead of the exact fp32 kernel — faster, differs by rounding")
    return p.parse_args(argv)


def main(argv=None):
    opt = parse_args(argv)
    if opt.wq_mfma16 and opt.use_aq:
        raise SystemExit("--wq_mfma16 selects a route of the weight-only state: it cannot be combined with --use_aq")
    if opt.wq_fused and opt.use_aq:
        raise SystemExit("--wq_fused selects a route of the weight-only state: it cannot be combined with --use_aq")
    if opt.wq_fused and not opt.wq_mfma16:
        raise SystemExit("--wq_fused folds into the matrix-core layers: it needs --wq_mfma16")
    if opt.attn_mfma16 and opt.use_aq:
        raise SystemExit("--attn_mfma16 selects a route of the un-quantised attention: it cannot be combined with --use_aq")
    if opt.attn_mfma16 and not opt.fp16:
        raise SystemExit("--attn_mfma16 serves 16-bit tensors: it needs --fp16 (the fp32 state keeps its exact attention kernel; "
                         "--attn_mfma16_fp32 is its switch)")
    if opt.attn_mfma16_fp32 and opt.use_aq:
        raise SystemExit("--attn_mfma16_fp32 selects a route of the un-quantised attention: it cannot be combined with --use_aq")
    if opt.attn_mfma16_fp32 and opt.fp16:
        raise SystemExit("--attn_mfma16_fp32 serves the fp32 state: it cannot be combined with --fp16 (--attn_mfma16 is the 16-bit switch)")
    if opt.aq_real_time_block and not (opt.use_aq and opt.aq_real_time):       # (a bad command line exits before anything is built)
        raise SystemExit("--aq_real_time_block is a granularity of the real-time mode: it needs --use_aq --aq_real_time")
    if opt.aq_real_time_block not in (0, 32):
        raise SystemExit("--aq_real_time_block is 0 or 32")
    if opt.aq_real_time_format == "mxfp6" and not (opt.use_aq and opt.aq_real_time and opt.aq_real_time_block == 32 and opt.aq == 6):
        raise SystemExit("--aq_real_time_format mxfp6 is a format of the real-time block mode at 6 activation bits: it needs --use_aq "
                         "--aq_real_time --aq_real_time_block 32 and --aq 6")
    logging.basicConfig(level=logging.INFO)
    from .diffusers_rewrite import UNet2DConditionModel, ARCH
    from .quant import get_qmodel, Scaler
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    mt = opt.model_type
    steps = opt.num_inference_steps if opt.num_inference_steps > 0 else (4 if mt == "sdxl" else 25)
    guidance = 0.0 if mt == "sdxl" else 7.5                     # src/inference_qmodel.py:48-51
    torch.manual_seed(opt.seed)

    unet = UNet2DConditionModel(mt)
    if opt.unet_weights:
        unet.load_state_dict(torch.load(opt.unet_weights, map_location="cpu"))
    else:
        synth.load_synth_weights(unet, mt, 0)
    pipe = types.SimpleNamespace(unet=unet)
    res = ARCH[mt]["sample_size"]
    batch = 2 if guidance > 0 else 1
    ckpt = opt.cali_ckpt
    real_time = opt.use_aq and opt.aq_real_time
    if opt.aq_real_time and not opt.use_aq:
        raise SystemExit("--aq_real_time is a mode of the activation quantizers: it needs --use_aq")
    if ckpt is None:
        ckpt = "/tmp/dgq_cli_%s_w%da%dg%d_s%d%s.pth" % (mt, opt.wq, opt.aq, opt.group_num if opt.use_group else 1, steps,
                                                       "_wonly" if real_time else "")
        if rank == 0 and not os.path.exists(ckpt):
            synth.write_cali_ckpt(ckpt, mt, opt.wq, opt.aq, opt.group_num if opt.use_group else 1,
                                  num_slots=steps if opt.time_aware_aqtizer else 1, seed=0, batch=batch, res=res,
                                  start_peak=opt.t2i_start_peak, uniform_softmax=opt.use_aq and not opt.t2i_log_quant,
                                  with_act=opt.use_aq and not real_time)
        if world > 1:
            import torch.distributed as dist
            dist.init_process_group("nccl")
            dist.barrier()

    wq_params = {"bits": opt.wq, "channel_wise": True, "scaler": Scaler.MINMAX}
    aq_params = {"bits": opt.aq, "channel_wise": False, "scaler": Scaler.MINMAX, "leaf_param": opt.use_aq}
    if real_time:
        aq_params["real_time"] = True
        if opt.aq_real_time_block:
            aq_params["real_time_block"] = opt.aq_real_time_block
        if opt.aq_real_time_format != "int":
            aq_params["real_time_format"] = opt.aq_real_time_format
    softmax_aq_params = {"softmax_a_bit": opt.aq, "t2i_log_quant": opt.t2i_log_quant,
                         "t2i_real_time": opt.t2i_real_time, "t2i_start_peak": opt.t2i_start_peak, "log_max_1": False}
    time_aware = opt.time_aware_aqtizer if opt.use_aq else False
    qnn = get_qmodel(mt, pipe, ckpt, wq_params, opt.use_aq, aq_params, softmax_aq_params, opt.use_group,
                     num_inference_steps=steps, time_aware_aqtizer=time_aware, device=dev)
    qnn = qnn.half() if opt.fp16 else qnn.float()
    qnn = qnn.to(dev)
    qnn.disable_out_quantization()
    if opt.wq_mfma16:
        qnn.set_weight_only_mfma16(True)
    if opt.wq_fused:
        qnn.set_weight_only_fused(True)
    if opt.attn_mfma16:
        qnn.set_attention_mfma16(True)
    if opt.attn_mfma16_fp32:
        qnn.set_attention_mfma16_fp32(True)
    if opt.graphs:
        qnn.enable_graphs(True)
    dt = torch.float16 if opt.fp16 else torch.float32

    def unet_fn(x, t, ctx, **extra):
        return qnn(x, t, ctx, **extra)[0]

    outs = {}
    for i in shard_prompts(opt.n_prompts, rank, world):
        lat = synth.named_randn("latent", (1, 4, res, res), opt.seed + i).to(dev, dt)
        ctx = synth.named_randn("ctx|" + opt.prompt, (batch, 77, ARCH[mt]["ctx_dim"]), opt.seed + i).to(dev, dt)
        extra = None
        if mt == "sdxl":
            inp = synth.synth_inputs("sdxl", batch, opt.seed + i, res)
            extra = {"added_cond_kwargs": {"text_embeds": inp["text_embeds"].to(dev, dt), "time_ids": inp["time_ids"].to(dev, dt)}}
        outs[i] = denoise_loop(unet_fn, lat, ctx, steps, guidance=guidance, extra=extra).float().cpu()
        logging.info("prompt %d done: latent absmax %.4f", i, outs[i].abs().max().item())
    out = opt.out.format(rank=rank)
    torch.save(outs, out)
    logging.info("saved %s", out)


if __name__ == "__main__":
    main()
