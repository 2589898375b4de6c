"""The three tiny ViT-VQGAN cases at head widths 32 / 96 / 128 and their seeded parameters: shared by tools/make_golden_dim_head.py (which runs the
reference's own modules on them and writes tests/golden/vit_tiny_dh*.npz) and tests/test_dim_head_model_gpu.py (which runs this package on them).

The configs are oracle/vitvq_oracle.py TINY_CFG with another dim_head / heads / image size.  The parameters follow the distributions of
vitvq_oracle.make_params (numpy MT19937, not torch's RNG) but take their SHAPES from the module's own state_dict — make_params fixes inner = 64 * heads.
Position tables are not generated: they stay the modules' own."""
import copy
import math

import numpy as np
import torch

PARAM_SEED, IMAGE_SEED, BATCH = 11, 5, 2
#        name      dim_head heads image   (patch 8: N = 64 | 36 | 36; dh128: inner 256 != dim 128)
CASES = {"dh32": (32, 4, 64), "dh96": (96, 1, 48), "dh128": (128, 2, 48)}


def case_cfg(name: str) -> dict:
    import vitvq_oracle as O
    dh, heads, size = CASES[name]
    cfg = copy.deepcopy(O.TINY_CFG)
    cfg["image_size"] = size
    for tower in ("encoder", "decoder"):
        cfg[tower].update(heads=heads, dim_head=dh)
    return cfg


def make_params(shapes: dict, cfg: dict, seed: int = PARAM_SEED) -> dict:
    """{name: tensor} for every entry of `shapes` ({state_dict key: shape}) except the position tables, drawn in sorted-key order"""
    rs = np.random.RandomState(seed)
    P = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith("pos_embedding"):
            continue
        if k == "quantizer.embedding.weight":
            a = rs.standard_normal(shp)
        elif k.startswith("pre_quant") or k.startswith("post_quant"):
            b = 1.0 / math.sqrt(cfg["encoder"]["dim"] if k.startswith("pre_quant") else cfg["quantizer"]["embed_dim"])
            a = rs.uniform(-b, b, shp)
        elif k.endswith("norm.weight"):
            a = 1.0 + 0.05 * rs.standard_normal(shp)
        elif k.endswith("bias"):
            a = 0.02 * rs.standard_normal(shp)
        else:  # xavier-uniform on the weight viewed [shape[0], -1]
            b = math.sqrt(6.0 / (int(np.prod(shp[1:])) + shp[0]))
            a = rs.uniform(-b, b, shp)
        P[k] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return P


def qkv_sample_rows(n_rows: int) -> np.ndarray:
    """the rows of encoder layer 0's to_qkv gradient that a golden file stores (at most 192, evenly spaced: q, k and v rows of every head)"""
    return np.arange(0, n_rows, max(-(-n_rows // 192), 1))
