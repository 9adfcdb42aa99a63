#!/usr/bin/env python3
"""Differential replay of the conv2d launch decision (tests/golden/conv_plans.json, tests/test_host.py).

Enumerates a deterministic grid of conv2d requests and records for each the outcome

    (tile code, split-K passed to madm_conv2d_fwd, post-GroupNorm carried, workspace bytes, tuned row found)

through one of two adapters over a library opened by path with plain ctypes (host code only, no GPU):

    --api old   the call sequence ops.conv2d made up to ABI 5: madm_conv2d_suggest_splitk with splitk = 1 and no stats -> set
                splitk -> madm_conv2d_can_post_groupnorm -> set pn_gamma or stats -> madm_conv2d_workspace_bytes,
                madm_conv2d_pick_tile, madm_conv2d_has_tuned_row
    --api new   one madm_conv2d_make_plan (ABI 6)

The fixture was written with ``--api old`` from a build of the last ABI-5 commit; the test replays it with ``new``.  After a change
that MEANS to move launches (new tuned rows, a new tile, another eligibility rule) regenerate it with ``--api new --write`` and
review the diff of the explicit cases.

The grid: every (M, N, K, KH, variant) of igemm_tuned.inc / igemm_tuned_latency.inc and the same shape at 2 M and M / 2 (off the
tables: heuristics, h16_pays), each with the geometries that factor M (B in 1, 2, 4; square and 1:2 maps; M x 1 for linear layers;
upsample geometry for variant 2, stride 2 for variant 3, gn_sums1 for variant 1), one and two sources, f32 / bf16 / f16, both
tuning profiles, tile override 0, -1, 12, 13 and 1 (no table row names tile 1: only the override reaches it), stats / post-GN /
residual / rowvec on and off, split-K chosen / forced 1 / forced 4.  The linear shapes run once more with one source under each of
epilogue = GEGLU, out_f32 and ln_colsum, crossed with everything but residual / rowvec.
"""
import argparse
import ctypes
import hashlib
import json
import math
import os
import re
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plans.json")
c_int, c_size_t = ctypes.c_int, ctypes.c_size_t


def _header_structs():
    """madm_conv2d_args / madm_conv2d_plan as include/madm_hip.h declares them.  madm_amd/_cabi.py is loaded by path: importing the
    package would load ITS library, and this tool opens the one it is given."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_cabi", os.path.join(ROOT, "madm_amd", "_cabi.py"))
    cabi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cabi)
    abi = cabi.parse_packaged("madm_hip.h")
    return abi.struct("madm_conv2d_args"), abi.struct("madm_conv2d_plan")


Args, Plan = _header_structs()

PTR = 64                                  # stands for "a tensor is given": the decision never looks behind a pointer
OVERRIDES = (0, -1, 12, 13, 1)
MODES = ("", "geglu", "out_f32", "ln")    # the extra flags of the linear shapes
SPLITK = (0, 1, 4)                        # 0 = the library chooses
GROUPS = 32
THIN = 39989                              # every THIN-th case of the grid is kept explicitly
FIELDS = ("override profile dtype B IH IW OH OW KH stride pad upsample C1 C2 N gn mode residual rowvec stats post_gn splitk "
          "tile splitk_passed post_gn_carried workspace_bytes row_found").split()


def open_lib(path, api):
    lib = ctypes.CDLL(path)
    pa = ctypes.POINTER(Args)
    names = {"old": ("suggest_splitk", "can_post_groupnorm", "pick_tile", "has_tuned_row", "workspace_bytes"),
             "new": ("make_plan",)}[api]
    for n in names:
        fn = getattr(lib, "madm_conv2d_" + n)
        fn.argtypes = [pa, ctypes.POINTER(Plan)] if n == "make_plan" else [pa]
        fn.restype = c_size_t if n == "workspace_bytes" else c_int
    lib.madm_set_tuning_profile.argtypes = lib.madm_debug_set_conv_tile.argtypes = [c_int]
    lib.madm_debug_set_conv_tile.restype = None
    return lib


def adapter(lib, api):
    """(args, splitk request, stats wanted, pn_groups) -> outcome; ``args`` carries everything else of the request."""
    if api == "new":
        plan = Plan()
        make_plan, pa, pp = lib.madm_conv2d_make_plan, ctypes.byref, ctypes.byref(plan)

        def new(a, sk, stats, groups):
            a.splitk, a.stats, a.pn_groups = sk, (PTR if stats else None), groups
            assert make_plan(pa(a), pp) == 0
            return plan.tile, plan.splitk, plan.post_gn, plan.workspace_bytes, plan.tuned_row
        return new
    suggest, can_post, pick = lib.madm_conv2d_suggest_splitk, lib.madm_conv2d_can_post_groupnorm, lib.madm_conv2d_pick_tile
    has_row, ws_bytes = lib.madm_conv2d_has_tuned_row, lib.madm_conv2d_workspace_bytes

    def old(a, sk, stats, groups):
        p = ctypes.byref(a)
        a.stats = a.pn_gamma = None
        a.pn_groups = 0
        a.splitk = 1
        if sk == 0:
            sk = suggest(p)
        a.splitk = max(1, sk)
        applied = False
        if groups:
            a.pn_groups = groups
            if can_post(p):
                a.pn_gamma = PTR
                applied = True
        if stats and not applied:
            a.stats = PTR
        return pick(p), a.splitk, int(applied), (ws_bytes(p) if a.splitk > 1 else 0), has_row(p)
    return old


def table_shapes():
    rows = set()
    for name in ("igemm_tuned.inc", "igemm_tuned_latency.inc"):
        for ln in open(os.path.join(ROOT, "madm_amd", "csrc", name)):
            m = re.match(r"^\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", ln)
            if m:
                rows.add(tuple(int(x) for x in m.groups()[1:6]))
    shapes = set()
    for M, N, K, KH, variant in rows:
        shapes.update((m, N, K, KH, variant) for m in ((M, 2 * M) if M % 2 else (M // 2, M, 2 * M)))
    return sorted(shapes)


def geometries(M, KH, variant):
    """(B, IH, IW, OH, OW, KH, stride, pad, upsample) of every map of the grid with B OH OW == M"""
    out = []
    for B in (1, 2, 4):
        if M % B:
            continue
        hw = M // B
        maps = [(hw, 1)] if KH == 1 else []
        s = math.isqrt(hw)
        if s * s == hw:
            maps.append((s, s))
        s = math.isqrt(hw // 2)
        if 2 * s * s == hw:
            maps.append((s, 2 * s))
        for OH, OW in maps:
            if variant == 2:
                if OH % 2 == 0 and OW % 2 == 0:
                    out.append((B, OH // 2, OW // 2, OH, OW, KH, 1, 1, 1))
            elif variant == 3:
                out.append((B, 2 * OH, 2 * OW, OH, OW, KH, 2, 0, 0))
            else:
                out.append((B, OH, OW, OH, OW, KH, 1, KH // 2, 0))
    return out


def sources(ctot):
    """one source, and two where the channels split into multiples of the K tile"""
    out = [(ctot, 0)]
    if ctot % 128 == 0:
        out.append((ctot // 2, ctot // 2))
    elif ctot > 64 and ctot % 64 == 0:
        out.append((64, ctot - 64))
    return out


def fill(a, dtype, B, IH, IW, OH, OW, KH, stride, pad, upsample, C1, C2, N, gn, mode, residual, rowvec):
    ctypes.memset(ctypes.byref(a), 0, ctypes.sizeof(a))
    a.dtype, a.B, a.IH, a.IW, a.OH, a.OW, a.KH, a.KW, a.stride, a.upsample = dtype, B, IH, IW, OH, OW, KH, KH, stride, upsample
    a.pad_t = a.pad_l = pad
    a.C1, a.C2, a.N = C1, C2, N
    a.in1 = a.w = a.out = PTR
    a.in2 = PTR if C2 else None
    a.ldo = N // 2 if mode == "geglu" else N
    a.epilogue = 1 if mode == "geglu" else 0
    a.out_f32 = 1 if mode == "out_f32" else 0
    if mode == "ln":
        a.ln_colsum, a.ln_eps = PTR, 1e-5
    if gn:
        a.gn_sums1 = a.gn_gamma = a.gn_beta = PTR
        a.gn_sums2 = PTR if C2 else None
        a.gn_groups, a.gn_eps = GROUPS, 1e-5
    if residual:
        a.residual, a.ldr = PTR, a.ldo
    if rowvec:
        a.rowvec, a.ldrv = PTR, N


def run_grid(lib, api):
    """-> (number of cases, sha256 of the packed outcomes, the explicit cases, tiles reached, values each boolean took)"""
    call = adapter(lib, api)
    a = Args()
    sha = hashlib.sha256()
    pack = struct.Struct("<iiiqi").pack
    explicit, tiles, seen = [], set(), [set(), set(), set()]   # post-GN carried, split-K launch, row found
    n = 0
    shapes = [(s, geometries(s[0], s[3], s[4]), sources(s[2] // (s[3] * s[3]))) for s in table_shapes()]
    try:
        for override in OVERRIDES:
            lib.madm_debug_set_conv_tile(override)
            for profile in (0, 1):
                assert lib.madm_set_tuning_profile(profile) == 0
                for (M, N, K, KH, variant), geoms, srcs in shapes:
                    for geom in geoms:
                        for C1, C2 in srcs:
                            for mode in (MODES if KH == 1 and C2 == 0 else MODES[:1]):
                                for dtype in (0, 1, 2):
                                    for flags in range(4 if mode else 16):
                                        residual, rowvec = flags >> 2 & 1, flags >> 3 & 1
                                        fill(a, dtype, *geom, C1, C2, N, int(variant == 1), mode, residual, rowvec)
                                        for sk in SPLITK:
                                            out = call(a, sk, flags & 1, GROUPS * (flags >> 1 & 1))
                                            sha.update(pack(*out))
                                            tiles.add(out[0])
                                            seen[0].add(out[2]), seen[1].add(out[3] > 0), seen[2].add(out[4])
                                            if n % THIN == 0:
                                                explicit.append([override, profile, dtype, *geom, C1, C2, N, int(variant == 1), mode,
                                                                 residual, rowvec, flags & 1, flags >> 1 & 1, sk, *out])
                                            n += 1
    finally:
        lib.madm_debug_set_conv_tile(0)
        lib.madm_set_tuning_profile(0)
    return n, sha.hexdigest(), explicit, tiles, seen


def run_case(lib, api, case):
    """the outcome of one explicit case of the fixture (the process' tile override and profile are restored)"""
    override, profile, *req = case[:22]
    a = Args()
    fill(a, *req[:-3])
    lib.madm_debug_set_conv_tile(override)
    lib.madm_set_tuning_profile(profile)
    try:
        return list(adapter(lib, api)(a, req[-1], req[-3], GROUPS * req[-2]))
    finally:
        lib.madm_debug_set_conv_tile(0)
        lib.madm_set_tuning_profile(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "madm_amd", "libmadm_hip.so"))
    ap.add_argument("--api", choices=("old", "new"), default="new")
    ap.add_argument("--write", action="store_true", help="write tests/golden/conv_plans.json (default: compare with it)")
    args = ap.parse_args()
    assert "MADM_TUNED_FILE" not in os.environ, "MADM_TUNED_FILE changes the decisions the fixture records"
    n, sha, explicit, tiles, seen = run_grid(open_lib(args.lib, args.api), args.api)
    print(f"{n} cases, sha256 {sha}, tiles {sorted(tiles)}, post-GN {sorted(seen[0])}, split-K {sorted(seen[1])}, "
          f"row {sorted(seen[2])}, {len(explicit)} explicit")
    if args.write:
        with open(FIXTURE, "w") as f:
            f.write('{"cases": %d, "sha256": "%s", "fields": %s, "explicit": [\n' % (n, sha, json.dumps(FIELDS)))
            f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in explicit))
            f.write("\n]}\n")
    else:
        want = json.load(open(FIXTURE))
        bad = [(w, g) for w, g in zip(want["explicit"], explicit) if w != g]
        for w, g in bad[:20]:
            print("fixture", w, "\n    got", g)
        assert (n, sha) == (want["cases"], want["sha256"]) and not bad, "the decisions differ from the fixture"
        print("equal to the fixture")


if __name__ == "__main__":
    main()
