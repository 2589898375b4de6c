"""Writes tests/golden/vit_tiny_dh32.npz, _dh96.npz and _dh128.npz: the REFERENCE's own ViTEncoder / ViTDecoder / VectorQuantizer (loaded by file path
through oracle/_reference_loader.py, wired as its ViTVQ wires them, as oracle/make_golden.py::gold_vit_tiny does) on the three cases of
tests/dim_head_cases.py.  Run once where the reference tree is available:  python tools/make_golden_dim_head.py
The files hold data only: outputs, losses, gradient names / norms, three sampled gradient tensors and the state-dict names / shapes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "enhancing-transformers_amd")):
    sys.path.insert(0, p)
import _reference_loader as RL  # noqa: E402
import dim_head_cases as DC  # noqa: E402
import vitvq_oracle as O  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def gold(name: str) -> None:
    from enhancing.modules.stage1.layers import get_2d_sincos_pos_embed
    L, Q = RL.load_layers(), RL.load_quantizers()
    cfg = DC.case_cfg(name)
    size, patch, dim, ed = cfg["image_size"], cfg["patch_size"], cfg["encoder"]["dim"], cfg["quantizer"]["embed_dim"]
    torch.manual_seed(0)
    enc = L.ViTEncoder(image_size=size, patch_size=patch, **cfg["encoder"])
    dec = L.ViTDecoder(image_size=size, patch_size=patch, **cfg["decoder"])
    quant = Q.VectorQuantizer(**cfg["quantizer"])
    pre, post = torch.nn.Linear(dim, ed), torch.nn.Linear(ed, cfg["decoder"]["dim"])      # vitvqgan.py:38-39
    mods = {"encoder.": enc, "decoder.": dec, "quantizer.": quant, "pre_quant.": pre, "post_quant.": post}
    shapes = {pref + k: tuple(v.shape) for pref, m in mods.items() for k, v in m.state_dict().items()}
    P = DC.make_params(shapes, cfg)
    for pref, m in mods.items():
        own = m.state_dict()
        own.update({k[len(pref):]: v for k, v in P.items() if k.startswith(pref)})
        m.load_state_dict(own, strict=True)
    # position tables: the modules' own; the package's table must be the reference's
    grid = size // patch
    table = torch.from_numpy(get_2d_sincos_pos_embed(dim, grid)).float().unsqueeze(0)
    assert torch.equal(enc.en_pos_embedding, table) and torch.equal(dec.de_pos_embedding, table), name
    x = O.make_images(DC.IMAGE_SEED, DC.BATCH, size)
    h = pre(enc(x))
    zq, qloss, idx = quant(h)
    xrec = dec(post(zq))
    l2 = (xrec - x).pow(2).mean()
    loss = l2 + qloss
    loss.backward()
    grads = {pref + k: v.grad for pref, m in mods.items() for k, v in m.named_parameters() if v.grad is not None}
    names = sorted(grads)
    g_qkv = grads["encoder.transformer.layers.0.0.fn.to_qkv.weight"]
    rows = DC.qkv_sample_rows(g_qkv.shape[0])
    state_names = sorted(shapes)
    state_shapes = np.zeros((len(state_names), 4), dtype=np.int64)
    for i, k in enumerate(state_names):
        state_shapes[i, :len(shapes[k])] = shapes[k]
    path = os.path.join(GOLD, f"vit_tiny_{name}.npz")
    np.savez_compressed(path, param_seed=DC.PARAM_SEED, image_seed=DC.IMAGE_SEED, B=DC.BATCH,
                        h=h.detach().numpy(), idx=idx.numpy().astype(np.int16), xrec=xrec.detach().numpy(),
                        loss=loss.item(), qloss=qloss.item(), l2=l2.item(),
                        grad_names=np.array(names), grad_norms=np.array([grads[k].double().norm().item() for k in names]),
                        g_qkv0_rows=rows, g_qkv0=g_qkv[torch.from_numpy(rows)].numpy(),
                        g_pixel_w=grads["decoder.to_pixel.1.weight"].numpy(), g_codebook=grads["quantizer.embedding.weight"].numpy(),
                        state_names=np.array(state_names), state_shapes=state_shapes)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): loss {loss.item():.6f}, qloss {qloss.item():.6f}, codes used {len(torch.unique(idx))}, "
          f"{len(names)} gradients")


if __name__ == "__main__":
    assert RL.available(), "needs the reference tree (ENH_REFERENCE_ROOT)"
    for name in DC.CASES:
        gold(name)
