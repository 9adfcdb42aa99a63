#!/usr/bin/env python3
"""Share of a tile's life that the LDS-DMA igemm spends behind its last MFMA (GLDS_STAMPS build, block 0 / wave 0): the
block-level stamps of igemm_glds_kernel -- [0] entry, [1] set-up done, [2] prologue DMA issued, [3] K loop done, [4] epilogue
issued -- for the short-K linear layers of the extract workload, f16, planned as the throughput profile plans them.
MADM_HIP_LIB=madm_amd/libmadm_hip_STAMPS.so python tools/exp/stamps_glds_epilogue.py [label]"""
import ctypes
import math
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from madm_amd import ops, packing

SHAPES = [  # M, N, K, form
    (8192, 2560, 320, "geglu"), (8192, 320, 320, "res"), (8192, 960, 320, "ln"),
    (2048, 5120, 640, "geglu"), (512, 1280, 1280, "res"), (8192, 320, 1600, "res"),
]
label = sys.argv[1] if len(sys.argv) > 1 else ""
read = getattr(ctypes.CDLL(os.environ["MADM_HIP_LIB"]), "madm_debug_read_glds_stamps")
read.restype = ctypes.c_int
dt = torch.float16
print(f"# {label} M N K form kernel: setup prologue loop epilogue total clocks, epilogue share of tile life")
for M, N, K, form in SHAPES:
    x = torch.randn((M, K), device="cuda").to(dt)
    w = torch.randn((N, K)) / math.sqrt(K)
    kw = {}
    if form == "ln":
        wp, bp, cs = packing.fold_layernorm(w, torch.zeros(N), torch.ones(K), torch.zeros(K), dt, ops.k_tile(dt))
        kw = dict(bias=bp.cuda(), ln=(cs.cuda(), 1e-5))
        wp = wp.cuda()
    else:
        wp = w.to(dt).cuda()
        kw = dict(bias=torch.randn(N, device="cuda"))
    if form == "geglu":
        kw["epilogue"] = ops.EPI_GEGLU
    if form == "res":
        kw["residual"] = torch.randn((M, N), device="cuda").to(dt)
    shares = []
    for rep in range(5):       # block 0 of five launches: the median share
        ops.PROFILE = []
        ops.linear(x, wp, B=2, **kw)
        torch.cuda.synchronize()
        kernel = ops.PROFILE[0][0]
        ops.PROFILE = None
        buf = (ctypes.c_ulonglong * 2048)()
        assert read(buf, 2048) == 0
        b = [buf[2000 + i] for i in range(5)]
        shares.append(((b[4] - b[3]) / max(1, b[4] - b[0]), b))
    shares.sort(key=lambda t: t[0])
    s, b = shares[len(shares) // 2]
    print(f"M{M} N{N} K{K} {form} {kernel}: {b[1] - b[0]} {b[2] - b[1]} {b[3] - b[2]} {b[4] - b[3]} {b[4] - b[0]}  {100 * s:.1f} %")
