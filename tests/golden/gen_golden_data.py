"""Writes tests/golden/data_samples.npz: what the REFERENCE's CrossModalityDataset returns on the tiny tree of
tests/data_util.py (``make_tree``) -- its outputs only, as arrays.  Run it where the reference checkout and PIL exist:

    python tests/golden/gen_golden_data.py

For every index the generators are seeded with ``data_util.seed_of(idx)`` right before ``__getitem__``; train samples come
from a dataset built with ``data_util.train_kwargs()``, evaluation samples from ``data_util.eval_kwargs()``.  Keys:
``{train|test}_{idx}_{tensor key}``, plus ``{mode}_{idx}_meta`` = (width, height)."""
import os
import random
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import data_util as du  # noqa: E402


def main():
    Ref = du.load_reference_class()
    out = {}
    with tempfile.TemporaryDirectory() as root:
        json_path, src, tgt = du.make_tree(root)
        for mode, kwargs, indices in (("train", du.train_kwargs(), du.TRAIN_INDICES), ("test", du.eval_kwargs(), du.EVAL_INDICES)):
            ds = Ref(json_path, src, tgt, **kwargs)
            for idx in indices:
                random.seed(du.seed_of(idx))
                np.random.seed(du.seed_of(idx))
                sample = ds[idx]
                for key in du.TENSOR_KEYS:
                    if key in sample:
                        out[du.golden_key(mode, idx, key)] = sample[key].numpy()
                out[du.golden_key(mode, idx, "meta")] = np.asarray([sample["width"], sample["height"]], dtype=np.int64)
    np.savez_compressed(du.GOLDEN, **out)
    print(f"wrote {du.GOLDEN}: {len(out)} arrays, {os.path.getsize(du.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
