"""The number the reference logs as val/total_loss for a stage-2 checkpoint: the mean cross-entropy of every code given the class and the codes
before it.  python tools/eval_gpt_nll.py -c configs/imagenet_gpt_vitvq_base.yaml --ckpt last.ckpt [--split validation | --synthetic N]

Builds the config's CondTransformer, loads `--ckpt` (a {"state_dict": ...} file; without it the config's own `path` entries or the random init are
used) and runs CondTransformer.validation_step (tokenizer -> teacher-forced GPT.forward or RQTransformer.forward -> device cross-entropy; an RQ
prior has depth_num_tokens codes per position) over the config's dataset split, or
over N images of the in-repo synthetic generator at the tokenizer's resolution.  Prints one JSON line: the mean NLL in nats per code (batches
weighted by their size), bits per code, and the counts."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing.utils.general import get_config_from_file, initialize_from_config  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--split", default="validation", choices=["train", "validation", "test"])
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate on this many synthetic images instead of the config's dataset")
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--max_batches", type=int, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_gpt_nll.py needs a ROCm device")
    cfg = get_config_from_file(args.config)
    model = initialize_from_config(cfg.model)
    if args.ckpt:
        model.init_from_ckpt(args.ckpt)
    if args.synthetic:
        from torch.utils.data import DataLoader
        from enhancing.dataloader.synthetic import SyntheticImages
        ds = SyntheticImages(resolution=cfg.model.params.stage1.params.image_size, length=args.synthetic, seed=1,
                             n_classes=model.transformer.vocab_cond_size)
        loader = DataLoader(ds, batch_size=args.batch_size or 4, num_workers=0)
    else:
        data = initialize_from_config(cfg.dataset)
        if args.batch_size:
            data.batch_size = args.batch_size
        data.setup()
        loader = {"train": data.train_dataloader, "validation": data.val_dataloader, "test": data.test_dataloader}[args.split]()
    total, codes, images = 0.0, 0, 0
    T = model.transformer.img_num_tokens * getattr(model.transformer, "depth_num_tokens", 1)      # codes per image (RQTransformer: D per position)
    for i, batch in enumerate(loader):
        if args.max_batches is not None and i >= args.max_batches:
            break
        batch = {k: v.cuda() if torch.is_tensor(v) else v for k, v in batch.items()}
        b = batch[model.stage1_model.image_key].shape[0]
        total += float(model.validation_step(batch, i)) * b * T
        codes += b * T
        images += b
    if not codes:
        raise SystemExit("eval_gpt_nll.py: the split is empty")
    nll = total / codes
    print(json.dumps({"val/total_loss": nll, "bits_per_code": nll / math.log(2), "images": images, "codes": codes,
                      "source": f"synthetic:{args.synthetic}" if args.synthetic else args.split}))


if __name__ == "__main__":
    main()
