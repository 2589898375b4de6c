"""Class-conditional image sampling with a stage-2 config:  python tools/sample_images.py -c configs/imagenet_gpt_vitvq_base.yaml --ckpt last.ckpt
--classes 207 360 --top_k 100 --top_p 0.95 --temperature 1.0 --seed 0 [--graph] [--weights fp8|fp6|fp4] [--cache fp8] --out samples.png
Image completion:  ... --complete photo1.png photo2.png --keep 0.5 --classes 207 360

Builds the config's CondTransformer (condition model, stage-1 tokenizer, and the prior: GPT, or RQTransformer over a residual tokenizer as in
configs/imagenet_rqtransformer_rqvae_base.yaml), loads `--ckpt` (a {"state_dict": ...} file; without it the config's own `path` entries or the
random init are used), samples one image per class id on the device and writes them as one PNG grid.  With --complete every given image is
tokenized by the stage 1, the top `--keep` of its token rows is kept and the rest is drawn once per class id (CondTransformer.complete: the kept
codes enter the caches through one batched prefill); the grid then has one row per image: the original, the kept part, the completions."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing.utils.callback import make_grid  # noqa: E402
from enhancing.utils.general import get_config_from_file, initialize_from_config  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
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
    ap.add_argument("--complete", nargs="+", default=None, metavar="IMAGE", help="image files to complete instead of sampling from nothing: one grid row per "
                    "image (the original, the kept part, one completion per class id)")
    ap.add_argument("--keep", type=float, default=0.5, help="with --complete: the fraction of the token rows, from the top, that is kept (default 0.5)")
    ap.add_argument("--nrow", type=int, default=4)
    ap.add_argument("--out", default="samples.png")
    return ap


def load_images(paths, size: int) -> torch.Tensor:
    """[n, 3, size, size] f32 in [0, 1]"""
    from PIL import Image
    imgs = [np.asarray(Image.open(p).convert("RGB").resize((size, size), Image.BICUBIC), dtype=np.float32) / 255.0 for p in paths]
    return torch.from_numpy(np.stack(imgs)).permute(0, 3, 1, 2).contiguous()


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not 0.0 <= args.keep < 1.0:
        raise SystemExit("--keep must be in [0, 1): at least one token row is left to draw")
    if not torch.cuda.is_available():
        raise SystemExit("sample_images.py needs a ROCm device")
    cfg = get_config_from_file(args.config)
    model = initialize_from_config(cfg.model)
    if args.ckpt:
        model.init_from_ckpt(args.ckpt)
    conds = torch.tensor(args.classes, dtype=torch.int64, device="cuda")
    kw = dict(top_k=args.top_k, top_p=args.top_p, softmax_temperature=args.temperature, use_fp16=not args.fp32, seed=args.seed,
              graph=True if args.graph else None, weights=args.weights, cache=args.cache)
    from PIL import Image
    if args.complete:
        originals = load_images(args.complete, int(cfg.model.params.stage1.params.image_size))
        n, k = len(args.complete), len(args.classes)
        # every image once per class id; row_offset-free: one call, so every (image, class) pair has its own uniforms
        done = model.complete(originals.repeat_interleave(k, 0).cuda(), conds.repeat(n), keep=args.keep, **kw).float().cpu()
        rows = int(model.code_shape[0]) if model.code_shape is not None else int(round(model.transformer.img_num_tokens ** 0.5))
        kept = originals.clone()
        kept[:, :, originals.shape[2] * int(args.keep * rows) // rows:] = 0.5      # the part that was drawn, greyed out
        img = torch.cat([torch.cat([originals[i:i + 1], kept[i:i + 1], done[i * k:(i + 1) * k]]) for i in range(n)])
        grid = make_grid(img, nrow=2 + k)
        Image.fromarray((grid.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(args.out)
        print(f"wrote {args.out}: {n} images {tuple(img.shape[1:])} completed for {k} classes, {int(args.keep * rows)} of {rows} token rows kept")
        return
    img = model.sample(conds, **kw)
    grid = make_grid(img.float().cpu(), nrow=args.nrow)
    Image.fromarray((grid.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(args.out)
    print(f"wrote {args.out}: {len(args.classes)} images {tuple(img.shape[1:])}")


if __name__ == "__main__":
    main()
