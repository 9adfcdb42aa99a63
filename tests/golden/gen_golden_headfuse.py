"""Fixtures of ``DAFormerHead(final_fuse_vae_decoder_feat=True)`` from the REFERENCE's own class (loaded by path through
oracle/ref_driver.load_modeling, CPU, float32), with seeded weights (weights.synth_init_ / synth_buffers_) and the seeded
inputs of tests/head_fuse_util.py:

  headfuse_eval.npz          eval forward, s0 128 x 64 x 64 and 512 x 8 x 8 / 4 x 4 / 2 x 2, B = 1, K = 11
  headfuse_eval_odd.npz      the same on 72 x 40 / 9 x 5 / 5 x 3 / 3 x 2
  headfuse_eval_odd_s0.npz   the same on 71 x 39 / ...: the classifier's resize is not a 2x
  headfuse_train.npz         train mode, B = 2, fixed Dropout2d scale: logits, all 46 parameter gradients and the four feature
                             gradients for a seeded dlogits (each as <= 2048 evenly spaced elements + its L2 norm), the
                             BatchNorm running statistics after the step
  headfuse_state.npz         the sorted state-dict keys with their shapes

Run where the reference lies (it is not needed to run the tests):  python tests/golden/gen_golden_headfuse.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import head_fuse_util as hu          # noqa: E402
from oracle import madm_path, ref_driver, train_path   # noqa: E402


def build():
    ns = ref_driver.load_modeling()
    head = ns.daformer_head.DAFormerHead(
        in_channels=list(hu.CHANNELS), in_keys=list(hu.KEYS), in_index=list(range(len(hu.KEYS))), channels=256,
        dropout_ratio=0.1, num_classes=hu.K, norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
        decoder_params=madm_path.head_decoder_params(), final_fuse_vae_decoder_feat=True)
    head.dropout = train_path.FixedDropout2d()
    return hu.init_head_(head)


def main():
    torch.set_num_threads(os.cpu_count())
    head = build()
    sd = head.state_dict()
    keys = sorted(sd)
    assert len(list(head.named_parameters())) == 46
    np.savez_compressed(os.path.join(HERE, "headfuse_state.npz"), keys=np.array(keys),
                        shapes=np.array([",".join(str(d) for d in sd[k].shape) for k in keys]))
    for name in hu.CASES:
        out = hu.run_case(build(), name)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, {k: v.shape for k, v in out.items() if k == "logits"}, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
