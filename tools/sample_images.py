"""Class-conditional image sampling with a stage-2 config:  python tools/sample_images.py -c configs/imagenet_gpt_vitvq_base.yaml --ckpt last.ckpt
--classes 207 360 --top_k 100 --top_p 0.95 --temperature 1.0 --seed 0 [--graph] [--weights fp8|fp6|fp4] [--cache fp8] --out samples.png

Builds the config's CondTransformer (condition model, stage-1 tokenizer, and the prior: GPT, or RQTransformer over a residual tokenizer as in
configs/imagenet_rqtransformer_rqvae_base.yaml), loads `--ckpt` (a {"state_dict": ...} file; without it the config's own `path` entries or the
random init are used), samples one image per class id on the device and writes them as one PNG grid."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing.utils.callback import make_grid  # noqa: E402
from enhancing.utils.general import get_config_from_file, initialize_from_config  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--classes", type=int, nargs="+", required=True)
    ap.add_argument("--top_k", type=int, default=None)
    ap.add_argument("--top_p", type=float, default=None)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fp32", action="store_true", help="the exact mode (use_fp16=False)")
    ap.add_argument("--graph", action="store_true", help="replay every position after the first from one captured HIP graph (sample(graph=True): "
                    "the same codes); without it ENH_GRAPHS=1 decides")
    ap.add_argument("--weights", choices=("h16", "fp8", "fp6", "fp4"), default=None, help="fp8: stream the Block weights as MXFP8 operands (sample(weights=\"fp8\"): half "
                    "the weight bytes of a step and of the operand copies); fp6: as MXFP6 operands (0.76 of fp8's bytes at fp8's accuracy on block-scaled weights, DESIGN.md "
                    "§3.16); fp4: as MXFP4 operands (a quarter; the format moves the logits far more, DESIGN.md §3.15); without it ENH_SAMPLE_WEIGHTS decides (default h16)")
    ap.add_argument("--cache", choices=("h16", "fp8"), default=None, help="fp8: hold the k / v caches as MXFP8 codes and scales (sample(cache=\"fp8\"): half "
                    "the cache bytes of a step and of device memory); without it ENH_SAMPLE_CACHE decides (default h16)")
    ap.add_argument("--nrow", type=int, default=4)
    ap.add_argument("--out", default="samples.png")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sample_images.py needs a ROCm device")
    cfg = get_config_from_file(args.config)
    model = initialize_from_config(cfg.model)
    if args.ckpt:
        model.init_from_ckpt(args.ckpt)
    conds = torch.tensor(args.classes, dtype=torch.int64, device="cuda")
    img = model.sample(conds, top_k=args.top_k, top_p=args.top_p, softmax_temperature=args.temperature, use_fp16=not args.fp32, seed=args.seed,
                       graph=True if args.graph else None, weights=args.weights, cache=args.cache)
    from PIL import Image
    grid = make_grid(img.float().cpu(), nrow=args.nrow)
    Image.fromarray((grid.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(args.out)
    print(f"wrote {args.out}: {len(args.classes)} images {tuple(img.shape[1:])}")


if __name__ == "__main__":
    main()
