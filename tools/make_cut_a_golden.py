#!/usr/bin/env python
"""Generate tests/golden/cut_a.npz: the REFERENCE's make_batch with cut_a=True (data_handler.py:219-274, the random answer
truncation at 255-260) on the deterministic mini-corpus of oracle.fixtures.det_corpus.

Runs only where the reference is present (as oracle/make_golden.py); the reference is imported, never copied.  Per case
(caption setting x seed x batch plan): np.random.seed(seed), then make_batch(..., cut_a=True) over a visiting sequence that
revisits batches (all batches in order, then a fixed permutation); per visit trg, trg_y, trg_mask and ntokens; at the end
np.random.get_state() (keys + position), so that a test can prove the stream was consumed identically.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_cut_a_golden.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.fixtures import det_corpus, save_golden  # noqa: E402
from oracle.make_golden import import_reference  # noqa: E402

SEEDS = (1, 7)
PLANS = ((4, 8), (6, 20))          # (batchsize, max_length) of make_batch_indices


def visits(n_batches):
    """All batches in order, then a fixed permutation of them (every batch visited twice)."""
    return list(range(n_batches)) + [int(k) for k in np.random.RandomState(100 + n_batches).permutation(n_batches)]


def main():
    import_reference()
    import data_handler as ref_dh        # noqa
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # the reference's prepare_data / Batch hard-code .cuda()
    out = {}
    try:
        for cap in (True, False):
            data = det_corpus(caption=cap)
            tmp = tempfile.mkdtemp(prefix="mtn_cut_a_")
            feats = []
            for fi, d in enumerate(data["features"]):
                fd = {}
                for vid, arr in d.items():
                    path = os.path.join(tmp, f"f{fi}_{vid}.npy")
                    np.save(path, arr)
                    fd[vid] = (path, arr.shape[0])
                feats.append(fd)
            ref_data = {"dialogs": data["dialogs"], "features": feats, "vocab": data["vocab"]}
            for bsz, mlen in PLANS:
                idx, _ = ref_dh.make_batch_indices(ref_data, batchsize=bsz, max_length=mlen, separate_caption=cap)
                seq = visits(len(idx))
                for seed in SEEDS:
                    tag = f"cap{int(cap)}.b{bsz}.s{seed}"
                    out[f"{tag}.visits"] = np.array(seq, dtype=np.int64)
                    np.random.seed(seed)
                    for v, k in enumerate(seq):
                        b = ref_dh.make_batch(ref_data, idx[k], data["vocab"], separate_caption=cap, cut_a=True)
                        for name in ("trg", "trg_y", "trg_mask"):
                            out[f"{tag}.{v}.{name}"] = getattr(b, name).numpy()
                        out[f"{tag}.{v}.ntokens"] = np.array(int(b.ntokens))
                    _, keys, pos, has_gauss, gauss = np.random.get_state()
                    out[f"{tag}.state_keys"], out[f"{tag}.state_pos"] = np.asarray(keys), np.array(pos)
                    out[f"{tag}.state_gauss"] = np.array([has_gauss, gauss], dtype=np.float64)
    finally:
        torch.Tensor.cuda = orig_cuda
    files = save_golden(os.path.join(ROOT, "tests", "golden", "cut_a.npz"), out)
    print("wrote", files, len(out), "arrays", [os.path.getsize(f) for f in files], "bytes")


if __name__ == "__main__":
    main()
