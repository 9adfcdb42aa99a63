// {dtype (0 f32, 1 bf16), M, N, K, KH, variant (0 plain, 1 GroupNorm-fused, 2 upsample, 3 stride 2), tile (1..17: the table g_tiles of igemm.hip), splitk}
// measured by tools/tune_insitu.py on MI355X (whole eager forwards, cold weights), bf16, round 1; plain and
// GroupNorm-fused variants come from runs under different fusion policies (ops.FUSE_GN_MAX_N)
// -- feature extractor, bs=2, 512x512 (BASELINE configs[1])
{1, 2, 1280, 320, 1, 0, 11, 1},   // r5 side-by-side: side 2.4 -> 2.1 us, alone 5.2 -> 4.1 (was tile 6)
{1, 2, 1280, 1280, 1, 0, 7, 8},
{1, 2, 20160, 1280, 1, 0, 7, 1},   // r5 side-by-side: side 9.1 -> 8.7 us, alone 14.0 -> 13.6 (was tile 11)
{1, 128, 1280, 1280, 1, 0, 7, 3},   // r4 side-by-side: side 4.9 -> 4.6 us, alone 8.6 -> 8.8 (was tile 7 sk4)
{1, 128, 1280, 2560, 1, 0, 7, 4},   // r3 retune: 13.0 vs 17.1 us (was tile 7 sk6)
{1, 128, 1280, 5120, 1, 0, 7, 6},
{1, 128, 1280, 11520, 3, 0, 11, 12},
{1, 128, 1280, 11520, 3, 1, 9, 24},
{1, 128, 1280, 23040, 3, 0, 8, 12},   // r3 retune: 31.6 vs 36.0 us (was tile 8 sk24)
{1, 128, 1280, 23040, 3, 1, 4, 24},
{1, 128, 3840, 1280, 1, 0, 7, 1},   // r4 side-by-side: side 23.4 -> 6.1 us, alone 24.8 -> 11.2 (was tile 13 sk1)
{1, 128, 10240, 1280, 1, 0, 8, 1},   // r4 side-by-side: side 9.9 -> 9.5 us, alone 17.5 -> 16.7 (was tile 11 sk1)
{1, 154, 24960, 768, 1, 0, 11, 1},
{1, 512, 640, 5760, 3, 0, 11, 6},
{1, 512, 1280, 640, 1, 0, 7, 1},   // r4 side-by-side: side 15.1 -> 3.9 us, alone 19.7 -> 7.5 (was tile 13 sk1)
{1, 512, 1280, 1280, 1, 0, 7, 1},
{1, 512, 1280, 1920, 1, 0, 7, 1},   // r4 side-by-side: side 9.6 -> 7.1 us, alone 14.0 -> 14.3 (was tile 11 sk3)
{1, 512, 1280, 2560, 1, 0, 7, 1},   // r4 side-by-side: side 10.4 -> 9.2 us, alone 16.4 -> 17.8 (was tile 8 sk3)
{1, 512, 1280, 5120, 1, 0, 8, 3},
{1, 512, 1280, 5760, 3, 0, 10, 3},   // r4 side-by-side: side 15.5 -> 13.3 us, alone 22.8 -> 24.2 (was tile 10 sk6)
{1, 512, 1280, 5760, 3, 1, 10, 6},
{1, 512, 1280, 11520, 3, 0, 10, 3},   // r4 side-by-side: side 22.8 -> 20.8 us, alone 32.4 -> 34.8 (was tile 10 sk6)
{1, 512, 1280, 11520, 3, 1, 10, 6},
{1, 512, 1280, 11520, 3, 2, 12, 8},   // r4 side-by-side: side 29.2 -> 21.5 us, alone 40.0 -> 39.5 (was tile 8 sk6)
{1, 512, 1280, 17280, 3, 0, 12, 8},   // r4 side-by-side: side 30.9 -> 27.3 us, alone 40.0 -> 47.9 (was tile 10 sk6)
{1, 512, 1280, 17280, 3, 1, 9, 6},
{1, 512, 1280, 23040, 3, 0, 12, 8},   // r4 side-by-side: side 37.9 -> 33.7 us, alone 51.3 -> 58.3 (was tile 10 sk6)
{1, 512, 1280, 23040, 3, 1, 9, 12},
{1, 512, 3840, 1280, 1, 0, 8, 1},   // r4 side-by-side: side 12.7 -> 10.4 us, alone 17.6 -> 16.5 (was tile 11 sk1)
{1, 512, 4096, 512, 1, 0, 8, 1},   // r4 side-by-side: side 6.3 -> 5.6 us, alone 9.5 -> 9.7 (was tile 11 sk1)
{1, 512, 10240, 1280, 1, 0, 15, 1},   // r5 side-by-side (GEGLU 16x16): side 26.4 -> 21.7 us, alone 36.1 -> 33.8 (was tile 2)
{1, 2048, 320, 2880, 3, 0, 7, 3},
{1, 2048, 640, 320, 1, 0, 11, 1},
{1, 2048, 640, 640, 1, 0, 11, 1},
{1, 2048, 640, 960, 1, 0, 11, 1},
{1, 2048, 640, 1280, 1, 0, 7, 1},
{1, 2048, 640, 1920, 1, 0, 7, 1},
{1, 2048, 640, 2560, 1, 0, 8, 1},   // r4 side-by-side: side 14.7 -> 12.4 us, alone 20.4 -> 24.9 (was tile 7 sk1)
{1, 2048, 640, 2880, 3, 0, 10, 1},   // r4 side-by-side: side 14.7 -> 10.9 us, alone 21.8 -> 22.3 (was tile 10 sk3)
{1, 2048, 640, 2880, 3, 1, 10, 3},
{1, 2048, 640, 5760, 3, 0, 10, 1},   // r4 side-by-side: side 21.9 -> 18.4 us, alone 30.8 -> 39.0 (was tile 10 sk3)
{1, 2048, 640, 5760, 3, 1, 9, 6},
{1, 2048, 640, 8640, 3, 0, 10, 3},
{1, 2048, 640, 8640, 3, 1, 10, 3},
{1, 2048, 640, 11520, 3, 0, 12, 4},   // r4 side-by-side: side 37.5 -> 32.6 us, alone 48.0 -> 56.7 (was tile 10 sk3)
{1, 2048, 640, 11520, 3, 1, 10, 3},
{1, 2048, 640, 17280, 3, 0, 12, 6},   // r5 (lean split-K epilogue of the 16x16 kernel): side 46.3 -> 44.6 us, alone 77.6 -> 58.8 (was sk4)
{1, 2048, 640, 17280, 3, 1, 9, 6},
{1, 2048, 1280, 11520, 3, 2, 12, 3},   // r4 side-by-side: side 101.1 -> 57.0 us, alone 122.3 -> 79.2 (tile 12 sk3; was tile 8 sk3)
{1, 2048, 1920, 640, 1, 0, 15, 1},   // r5 side-by-side (QKV 32x32): side 10.8 -> 9.2 us, alone 14.8 -> 14.9 (tile 17 in round 4)
{1, 2048, 5120, 640, 1, 0, 15, 1},   // r5 side-by-side (GEGLU 32x32): side 28.0 -> 23.7 us, alone 36.0 -> 31.8 (was tile 2)
{1, 4096, 512, 4096, 1, 0, 8, 1},   // r4 side-by-side: side 28.1 -> 24.4 us, alone 33.3 -> 38.0 (was tile 11 sk1)
{1, 4096, 4096, 512, 1, 0, 15, 1},   // r5 side-by-side: side 33.6 -> 30.0 us, alone 39.6 -> 31.3 (was tile 2 sk1)
{1, 8192, 4, 2880, 3, 1, 10, 8},   // r3 retune: 18.0 vs 25.8 us (was tile 9 sk12)
{1, 8192, 8, 4608, 3, 1, 10, 4},   // r4 side-by-side: side 11.7 -> 10.7 us, alone 21.5 -> 23.2 (was tile 10 sk24)
{1, 8192, 320, 320, 1, 0, 11, 1},
{1, 8192, 320, 576, 3, 0, 10, 1},   // r4 side-by-side: side 6.3 -> 6.1 us, alone 11.4 -> 11.1 (was tile 10 sk2)
{1, 8192, 320, 640, 1, 0, 8, 1},   // r4 side-by-side: side 7.8 -> 7.2 us, alone 11.3 -> 12.1 (was tile 11 sk1)
{1, 8192, 320, 960, 1, 0, 8, 1},   // r4 side-by-side: side 10.2 -> 9.3 us, alone 13.6 -> 15.0 (was tile 11 sk1)
{1, 8192, 320, 1280, 1, 0, 8, 1},   // r4 side-by-side: side 13.4 -> 12.1 us, alone 16.9 -> 17.9 (was tile 11 sk1)
{1, 8192, 320, 2880, 3, 0, 10, 1},
{1, 8192, 320, 2880, 3, 1, 10, 1},
{1, 8192, 320, 5760, 3, 0, 10, 1},
{1, 8192, 320, 5760, 3, 1, 10, 1},
{1, 8192, 320, 8640, 3, 0, 10, 1},   // r4 side-by-side: side 48.2 -> 42.4 us, alone 66.9 -> 62.6 (was tile 10 sk2)
{1, 8192, 320, 8640, 3, 1, 9, 4},
{1, 8192, 512, 512, 1, 0, 15, 1},   // r5 side-by-side: side 10.8 -> 10.0 us, alone 14.1 -> 13.5 (was tile 2)
{1, 8192, 512, 4608, 3, 0, 12, 1},   // r4 side-by-side: side 41.2 -> 33.0 us, alone 45.0 -> 66.3 (was tile 10 sk1)
{1, 8192, 512, 4608, 3, 1, 10, 1},
{1, 8192, 640, 5760, 3, 2, 12, 1},   // r4 side-by-side: side 114.1 -> 50.1 us, alone 116.6 -> 80.7 (was tile 11 sk1)
{1, 8192, 960, 320, 1, 0, 15, 1},   // r5 side-by-side (QKV 64x64): side 12.9 -> 12.1 us, alone 19.8 -> 15.6 (was tile 2)
{1, 8192, 1024, 512, 1, 0, 15, 1},   // r5 side-by-side: side 17.4 -> 14.5 us, alone 20.2 -> 15.9 (was tile 8)
{1, 8192, 2560, 320, 1, 0, 15, 1},   // r5 side-by-side (GEGLU 64x64): side 34.6 -> 29.8 us, alone 41.6 -> 34.3 (was tile 2)
{1, 32768, 256, 2304, 3, 0, 8, 1},
{1, 32768, 512, 256, 1, 0, 15, 1},   // r5 side-by-side: side 22.0 -> 20.8 us, alone 24.9 -> 21.9 (was tile 2)
{1, 32768, 512, 2304, 3, 0, 9, 1},
{1, 32768, 512, 2304, 3, 1, 9, 1},
{1, 32768, 512, 4608, 3, 0, 9, 1},
{1, 32768, 512, 4608, 3, 1, 9, 1},
{1, 131072, 128, 1152, 3, 0, 8, 1},   // r3 retune: 91.9 vs 105.0 us (was tile 2 sk1)
{1, 131072, 256, 128, 1, 0, 15, 1},   // r5 side-by-side: side 35.1 -> 33.4 us, alone 35.1 -> 31.3 (was tile 2)
{1, 131072, 256, 1152, 3, 0, 9, 1},
{1, 131072, 256, 1152, 3, 1, 9, 1},
{1, 131072, 256, 2304, 3, 0, 9, 1},
{1, 131072, 256, 2304, 3, 1, 9, 1},
{1, 524288, 128, 64, 1, 0, 2, 1},
{1, 524288, 128, 1152, 3, 1, 9, 1},
// -- full inference forward, bs=1, 512x512, RGB->Depth config (BASELINE configs[2]): additional shapes
{1, 1, 1280, 320, 1, 0, 11, 1},   // r5 side-by-side: side 3.6 -> 3.3 us, alone 5.3 -> 4.4 (was tile 6 sk1)
{1, 1, 1280, 1280, 1, 0, 7, 8},
{1, 1, 20160, 1280, 1, 0, 7, 1},   // r4 side-by-side: side 9.2 -> 8.9 us, alone 14.4 -> 13.9 (was tile 11 sk1)
{1, 64, 1280, 1280, 1, 0, 7, 1},   // r5 side-by-side: side 6.6 -> 5.3 us, alone 15.5 -> 11.0 (was tile 8 sk4)
{1, 64, 1280, 2560, 1, 0, 11, 8},   // r5 side-by-side: side 5.3 -> 5.1 us, alone 9.1 -> 8.8 (was tile 11 sk6)
{1, 64, 1280, 5120, 1, 0, 11, 24},
{1, 64, 1280, 11520, 3, 0, 11, 12},   // r4 side-by-side: side 10.1 -> 9.2 us, alone 16.5 -> 16.0 (was tile 7 sk24)
{1, 64, 1280, 11520, 3, 1, 5, 24},
{1, 64, 1280, 23040, 3, 0, 7, 24},
{1, 64, 1280, 23040, 3, 1, 10, 24},
{1, 64, 3840, 1280, 1, 0, 7, 2},   // r4 side-by-side: side 6.4 -> 6.0 us, alone 11.8 -> 10.6 (was tile 6 sk4)
{1, 64, 10240, 1280, 1, 0, 7, 1},
{1, 77, 24960, 768, 1, 0, 8, 1},
{1, 256, 128, 1152, 3, 1, 10, 2},   // r4 side-by-side: side 7.7 -> 5.7 us, alone 19.2 -> 12.4 (was tile 9 sk6)
{1, 256, 128, 1280, 1, 0, 11, 6},   // r4 side-by-side: side 4.2 -> 3.5 us, alone 8.7 -> 7.5 (was tile 8 sk6)
{1, 256, 256, 512, 1, 0, 7, 1},
{1, 256, 512, 128, 1, 0, 7, 1},
{1, 256, 512, 1280, 1, 0, 11, 8},
{1, 256, 640, 5760, 3, 0, 11, 12},
{1, 256, 1280, 640, 1, 0, 7, 1},
{1, 256, 1280, 1280, 1, 0, 7, 1},
{1, 256, 1280, 1920, 1, 0, 7, 3},
{1, 256, 1280, 2560, 1, 0, 7, 3},
{1, 256, 1280, 5120, 1, 0, 8, 6},
{1, 256, 1280, 5760, 3, 0, 10, 6},   // r4 side-by-side: side 12.2 -> 10.2 us, alone 19.1 -> 17.3 (was tile 5 sk16)
{1, 256, 1280, 5760, 3, 1, 10, 12},
{1, 256, 1280, 11520, 3, 0, 10, 6},   // r4 side-by-side: side 15.4 -> 13.7 us, alone 23.4 -> 24.5 (was tile 10 sk12)
{1, 256, 1280, 11520, 3, 1, 10, 12},
{1, 256, 1280, 11520, 3, 2, 8, 6},   // r4 side-by-side: side 17.8 -> 15.4 us, alone 25.7 -> 29.0 (was tile 8 sk12)
{1, 256, 1280, 17280, 3, 0, 10, 6},   // r4 side-by-side: side 19.9 -> 17.8 us, alone 28.9 -> 28.7 (was tile 10 sk12)
{1, 256, 1280, 17280, 3, 1, 10, 12},
{1, 256, 1280, 23040, 3, 0, 10, 6},   // r4 side-by-side: side 24.0 -> 22.1 us, alone 34.5 -> 36.6 (was tile 10 sk12)
{1, 256, 1280, 23040, 3, 1, 10, 12},
{1, 256, 3840, 1280, 1, 0, 11, 1},   // r5 side-by-side: side 7.8 -> 7.3 us, alone 12.1 -> 11.8 (was tile 7 sk1)
{1, 256, 10240, 1280, 1, 0, 15, 1},   // r5 side-by-side: side 15.6 -> 13.5 us, alone 25.3 -> 27.8 (was tile 8 sk1)
{1, 1024, 128, 640, 1, 0, 7, 1},
{1, 1024, 128, 1152, 3, 1, 10, 2},
{1, 1024, 256, 512, 1, 0, 7, 1},
{1, 1024, 320, 2880, 3, 0, 7, 3},
{1, 1024, 512, 128, 1, 0, 7, 1},
{1, 1024, 512, 640, 1, 0, 7, 1},
{1, 1024, 640, 320, 1, 0, 11, 1},
{1, 1024, 640, 640, 1, 0, 7, 1},
{1, 1024, 640, 960, 1, 0, 7, 1},
{1, 1024, 640, 1280, 1, 0, 7, 1},
{1, 1024, 640, 1920, 1, 0, 7, 1},
{1, 1024, 640, 2560, 1, 0, 11, 2},
{1, 1024, 640, 2880, 3, 0, 10, 1},   // r4 side-by-side: side 11.0 -> 9.4 us, alone 17.4 -> 21.8 (was tile 10 sk16)
{1, 1024, 640, 2880, 3, 1, 10, 8},
{1, 1024, 640, 5760, 3, 0, 10, 3},   // r4 side-by-side: side 15.1 -> 13.4 us, alone 22.8 -> 24.3 (was tile 10 sk6)
{1, 1024, 640, 5760, 3, 1, 10, 6},
{1, 1024, 640, 8640, 3, 0, 10, 3},   // r4 side-by-side: side 19.2 -> 17.6 us, alone 28.7 -> 28.8 (was tile 10 sk6)
{1, 1024, 640, 8640, 3, 1, 10, 6},
{1, 1024, 640, 11520, 3, 0, 10, 3},   // r4 side-by-side: side 23.3 -> 21.5 us, alone 33.4 -> 35.3 (was tile 10 sk6)
{1, 1024, 640, 11520, 3, 1, 9, 12},
{1, 1024, 640, 17280, 3, 0, 12, 8},   // r4 side-by-side: side 30.8 -> 27.2 us, alone 40.7 -> 47.9 (was tile 10 sk6)
{1, 1024, 640, 17280, 3, 1, 10, 6},
{1, 1024, 1280, 11520, 3, 2, 12, 4},   // r4 side-by-side: side 48.0 -> 33.2 us, alone 61.6 -> 57.2 (was tile 8 sk3)
{1, 1024, 1920, 640, 1, 0, 11, 1},
{1, 1024, 5120, 640, 1, 0, 15, 1},   // r5 side-by-side: side 15.1 -> 12.9 us, alone 21.8 -> 20.8 (was tile 2 sk1)
{1, 4096, 4, 64, 1, 0, 11, 1},
{1, 4096, 4, 2880, 3, 1, 10, 6},
{1, 4096, 8, 4608, 3, 1, 10, 8},
{1, 4096, 128, 320, 1, 0, 11, 1},
{1, 4096, 128, 1152, 3, 1, 10, 1},
{1, 4096, 256, 512, 1, 0, 7, 1},
{1, 4096, 320, 320, 1, 0, 11, 1},   // r4 side-by-side: side 3.5 -> 3.2 us, alone 6.7 -> 6.5 (was tile 7 sk1)
{1, 4096, 320, 576, 3, 0, 6, 1},
{1, 4096, 320, 640, 1, 0, 11, 1},
{1, 4096, 320, 960, 1, 0, 7, 1},
{1, 4096, 320, 1280, 1, 0, 7, 1},
{1, 4096, 320, 2880, 3, 0, 10, 1},
{1, 4096, 320, 2880, 3, 1, 10, 3},
{1, 4096, 320, 5760, 3, 0, 10, 1},   // r4 side-by-side: side 20.8 -> 17.8 us, alone 33.0 -> 37.1 (was tile 10 sk3)
{1, 4096, 320, 5760, 3, 1, 10, 3},
{1, 4096, 320, 8640, 3, 0, 10, 3},
{1, 4096, 320, 8640, 3, 1, 10, 3},
{1, 4096, 512, 128, 1, 0, 7, 1},
{1, 4096, 512, 320, 1, 0, 11, 1},
{1, 4096, 512, 512, 1, 0, 2, 1},   // r4 side-by-side: side 6.3 -> 5.0 us, alone 8.2 -> 10.4 (was tile 7 sk1)
{1, 4096, 512, 576, 3, 0, 10, 4},
{1, 4096, 512, 4608, 3, 0, 10, 1},
{1, 4096, 512, 4608, 3, 1, 9, 4},
{1, 4096, 640, 5760, 3, 2, 12, 2},   // r4 side-by-side: side 51.2 -> 32.9 us, alone 62.9 -> 56.9 (was tile 11 sk1)
{1, 4096, 960, 320, 1, 0, 15, 1},   // r5 side-by-side: side 8.1 -> 6.6 us, alone 10.8 -> 10.7 (was tile 8 sk1)
{1, 4096, 1024, 512, 1, 0, 15, 1},   // r5 side-by-side: side 9.1 -> 7.3 us, alone 11.2 -> 11.4 (was tile 8 sk1)
{1, 4096, 2560, 320, 1, 0, 15, 1},   // r5 side-by-side: side 17.8 -> 16.4 us, alone 23.5 -> 22.3 (was tile 2 sk1)
{1, 16384, 256, 2304, 3, 0, 8, 1},
{1, 16384, 512, 256, 1, 0, 15, 1},   // r5 side-by-side: side 11.3 -> 10.5 us, alone 15.6 -> 12.5 (was tile 2 sk1)
{1, 16384, 512, 2304, 3, 0, 12, 1},   // r4 side-by-side: side 44.1 -> 31.5 us, alone 52.7 -> 43.5 (was tile 9 sk1)
{1, 16384, 512, 2304, 3, 1, 9, 1},
{1, 16384, 512, 4608, 3, 0, 12, 1},   // r4 side-by-side: side 76.2 -> 59.4 us, alone 82.1 -> 71.7 (was tile 9 sk1)
{1, 16384, 512, 4608, 3, 1, 9, 1},
{1, 16384, 512, 4608, 3, 2, 12, 1},   // r4 side-by-side: side 109.7 -> 58.5 us, alone 127.2 -> 73.2 (was tile 8 sk1)
{1, 65536, 128, 1152, 3, 0, 8, 1},
{1, 65536, 256, 128, 1, 0, 2, 1},   // r4 side-by-side: side 21.2 -> 20.4 us, alone 22.0 -> 20.3 (was tile 3 sk1)
{1, 65536, 256, 512, 1, 0, 15, 1},   // r5 side-by-side: side 36.1 -> 31.7 us, alone 38.5 -> 32.6 (was tile 2 sk1)
{1, 65536, 256, 1152, 3, 0, 10, 1},
{1, 65536, 256, 1152, 3, 1, 9, 1},
{1, 65536, 256, 2304, 3, 0, 9, 1},
{1, 65536, 256, 2304, 3, 1, 9, 1},
{1, 65536, 256, 4608, 3, 0, 9, 1},
{1, 65536, 256, 4608, 3, 1, 9, 1},
{1, 65536, 512, 4608, 3, 2, 12, 1},   // r5 side-by-side: side 503.3 -> 232.5 us, alone 479.8 -> 244.6 (was tile 2 sk1)
{1, 262144, 4, 1152, 3, 1, 10, 1},
{1, 262144, 12, 256, 1, 0, 3, 1},
{1, 262144, 128, 64, 1, 0, 15, 1},   // r5 side-by-side: side 29.7 -> 27.9 us, alone 30.1 -> 29.0 (was tile 2 sk1)
{1, 262144, 128, 128, 1, 0, 15, 1},   // r5 side-by-side: side 37.9 -> 35.3 us, alone 36.3 -> 35.0 (was tile 2 sk1)
{1, 262144, 128, 256, 1, 0, 15, 1},   // r5 side-by-side: side 50.1 -> 47.4 us, alone 60.4 -> 55.0 (was tile 2 sk1)
{1, 262144, 128, 1152, 3, 1, 9, 1},
{1, 262144, 128, 2304, 3, 1, 9, 1},
{1, 262144, 256, 128, 1, 0, 15, 1},   // r5 side-by-side: side 73.8 -> 69.6 us, alone 66.4 -> 58.1 (was tile 2 sk1)
{1, 262144, 256, 1024, 1, 0, 15, 1},   // r5 side-by-side: side 251.7 -> 204.3 us, alone 268.0 -> 216.5 (was tile 2 sk1)
{1, 262144, 256, 2304, 3, 2, 12, 1},   // r5 side-by-side: side 510.1 -> 242.9 us, alone 509.4 -> 251.5 (was tile 2 sk1)
{1, 262144, 256, 9216, 3, 0, 9, 1},
// -- round 4: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 128, 1280, 11520, 3, 3, 7, 6},   // r4 side-by-side: side 13.5 -> 12.2 us, alone 20.0 -> 21.2
{1, 128, 1280, 6400, 1, 0, 11, 6},   // r4 side-by-side: side 11.0 -> 8.7 us, alone 18.0 -> 14.0
{1, 512, 1280, 6400, 1, 0, 14, 3},   // r4 side-by-side: side 23.0 -> 17.1 us, alone 33.9 -> 34.8
{1, 2048, 640, 3200, 1, 0, 8, 1},   // r4 side-by-side: side 18.3 -> 14.7 us, alone 32.1 -> 30.1
{1, 8192, 512, 4608, 3, 3, 15, 1},   // r4 side-by-side: side 63.7 -> 48.7 us, alone 76.1 -> 71.7
{1, 32768, 256, 2304, 3, 3, 15, 1},   // r4 side-by-side: side 73.2 -> 59.3 us, alone 83.8 -> 59.5
{1, 131072, 128, 1152, 3, 3, 15, 1},   // r5 side-by-side: side 76.2 -> 64.7 us, alone 86.4 -> 66.8 (tile 8 in round 4, tile 15 before)
// -- round 4: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 64, 1280, 6400, 1, 0, 7, 6},   // r4 side-by-side: side 9.0 -> 7.3 us, alone 16.2 -> 13.1
{1, 64, 1280, 11520, 3, 3, 7, 12},   // r4 side-by-side: side 10.0 -> 9.4 us, alone 16.4 -> 15.5
{1, 256, 640, 5760, 3, 3, 11, 6},   // r4 side-by-side: side 9.3 -> 8.1 us, alone 15.1 -> 15.3
{1, 256, 1280, 6400, 1, 0, 14, 6},   // r4 side-by-side: side 14.7 -> 11.8 us, alone 23.5 -> 23.0
{1, 1024, 640, 3200, 1, 0, 7, 1},   // r4 side-by-side: side 13.6 -> 10.4 us, alone 20.2 -> 21.0
{1, 4096, 320, 1600, 1, 0, 11, 1},   // r4 side-by-side: side 10.2 -> 8.5 us, alone 18.9 -> 14.3
// -- round 4: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 192, 1280, 1280, 1, 0, 7, 1},   // r4 side-by-side: side 6.4 -> 4.9 us, alone 11.9 -> 10.7
{1, 192, 1280, 2560, 1, 0, 11, 4},   // r5 side-by-side: side 6.6 -> 6.3 us, alone 12.3 -> 11.8 (was tile 11 sk3)
{1, 192, 1280, 11520, 3, 0, 10, 4},   // r4 side-by-side: side 18.1 -> 15.3 us, alone 29.6 -> 27.3
{1, 192, 1280, 11520, 3, 3, 8, 6},   // r4 side-by-side: side 18.9 -> 15.7 us, alone 29.7 -> 29.1
{1, 192, 1280, 23040, 3, 0, 15, 12},   // r5 side-by-side: side 27.4 -> 26.2 us, alone 46.3 -> 41.2 (was tile 8 sk6)
{1, 768, 640, 5760, 3, 3, 8, 3},   // r4 side-by-side: side 17.0 -> 14.0 us, alone 27.1 -> 28.8
{1, 768, 1280, 1280, 1, 0, 11, 1},   // r4 side-by-side: side 7.7 -> 6.5 us, alone 15.2 -> 11.2
{1, 768, 1280, 1920, 1, 0, 11, 1},   // r4 side-by-side: side 11.0 -> 8.7 us, alone 25.0 -> 15.5
{1, 768, 1280, 2560, 1, 0, 11, 1},   // r4 side-by-side: side 14.2 -> 11.4 us, alone 34.0 -> 20.0
{1, 768, 1280, 5760, 3, 0, 10, 1},   // r4 side-by-side: side 30.7 -> 17.8 us, alone 77.9 -> 39.0
{1, 768, 1280, 6400, 1, 0, 14, 2},   // r4 side-by-side: side 31.4 -> 23.8 us, alone 78.4 -> 45.9
{1, 768, 1280, 11520, 3, 0, 12, 6},   // r4 side-by-side: side 57.3 -> 29.3 us, alone 149.2 -> 50.2
{1, 768, 1280, 11520, 3, 2, 12, 8},   // r4 side-by-side: side 56.0 -> 28.5 us, alone 148.4 -> 45.4
{1, 768, 1280, 17280, 3, 0, 12, 6},   // r4 side-by-side: side 83.4 -> 36.9 us, alone 192.7 -> 58.2
{1, 768, 1280, 23040, 3, 0, 12, 6},   // r4 side-by-side: side 108.4 -> 46.5 us, alone 296.8 -> 77.4
{1, 3072, 320, 2880, 3, 3, 11, 1},   // r4 side-by-side: side 15.5 -> 11.9 us, alone 32.2 -> 25.3
{1, 3072, 640, 640, 1, 0, 8, 1},   // r4 side-by-side: side 5.9 -> 5.4 us, alone 11.2 -> 10.9
{1, 3072, 640, 1920, 1, 0, 8, 1},   // r4 side-by-side: side 15.1 -> 12.9 us, alone 22.4 -> 21.2
{1, 3072, 640, 2880, 3, 0, 10, 1},   // r4 side-by-side: side 34.6 -> 14.2 us, alone 46.2 -> 23.4
{1, 3072, 640, 3200, 1, 0, 8, 1},   // r4 side-by-side: side 24.2 -> 20.0 us, alone 32.5 -> 31.4
{1, 3072, 640, 5760, 3, 0, 10, 1},   // r4 side-by-side: side 44.1 -> 25.1 us, alone 61.0 -> 38.7
{1, 3072, 640, 8640, 3, 0, 10, 1},   // r5 side-by-side: side 36.2 -> 34.1 us, alone 55.4 -> 55.4 (was tile 12 sk3)
{1, 3072, 640, 11520, 3, 0, 12, 4},   // r4 side-by-side: side 66.6 -> 45.1 us, alone 95.5 -> 64.0
{1, 3072, 640, 17280, 3, 0, 12, 4},   // r4 side-by-side: side 88.8 -> 60.8 us, alone 127.5 -> 88.4
{1, 3072, 1280, 11520, 3, 2, 12, 2},   // r4 side-by-side: side 126.1 -> 77.8 us, alone 144.8 -> 105.3
{1, 12288, 8, 4608, 3, 1, 10, 4},   // r4 side-by-side: side 17.4 -> 14.1 us, alone 36.0 -> 26.2
{1, 12288, 320, 2880, 3, 0, 10, 1},   // r5 side-by-side: side 24.3 -> 23.2 us, alone 44.0 -> 29.3 (was tile 12 sk1)
{1, 12288, 320, 5760, 3, 0, 10, 1},   // r5 side-by-side: side 46.7 -> 42.7 us, alone 81.3 -> 51.6 (was tile 12 sk1)
{1, 12288, 320, 8640, 3, 0, 10, 1},   // r5 side-by-side: side 69.3 -> 63.0 us, alone 119.1 -> 73.0 (was tile 12 sk1)
{1, 12288, 512, 4608, 3, 0, 12, 1},   // r4 side-by-side: side 65.7 -> 45.1 us, alone 84.1 -> 68.6
{1, 12288, 512, 4608, 3, 3, 15, 1},   // r4 side-by-side: side 90.3 -> 78.3 us, alone 111.6 -> 88.7
{1, 12288, 640, 5760, 3, 2, 12, 1},   // r4 side-by-side: side 127.3 -> 66.4 us, alone 145.4 -> 84.6
{1, 12288, 960, 320, 1, 0, 15, 1},   // r5 side-by-side: side 19.8 -> 18.3 us, alone 26.1 -> 23.9 (was tile 2 sk1)
{1, 49152, 256, 2304, 3, 3, 15, 1},   // r4 side-by-side: side 97.4 -> 93.2 us, alone 106.8 -> 98.4
// -- round 4: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 512, 640, 5760, 3, 3, 8, 6},   // r4 side-by-side: side 12.6 -> 11.2 us, alone 18.9 -> 19.7
{1, 2048, 320, 2880, 3, 3, 7, 1},   // r4 side-by-side: side 11.9 -> 10.2 us, alone 20.8 -> 24.7
// -- training step, bs=2, 512x512, RGB->Depth config (BASELINE configs[3]): shapes of the data gradients / head / decoder that the
//    tables above do not hold (tools/tune_concurrent.py --workload train --streams 1: eager launches on one stream)
{1, 524288, 256, 1024, 1, 0, 15, 1},   // r4 train step, lone launch: one stream 495.6 -> 411.5 us, alone 505.8 -> 408.5
{1, 524288, 1024, 256, 1, 0, 15, 1},   // r4 train step, lone launch: one stream 932.1 -> 857.1 us, alone 932.5 -> 853.9
{1, 2048, 640, 5120, 1, 0, 14, 3},   // r4 train step, lone launch: one stream 61.1 -> 30.3 us, alone 60.5 -> 30.1
{1, 512, 2560, 11520, 3, 0, 9, 3},   // r4 train step, lone launch: one stream 157.4 -> 50.2 us, alone 156.4 -> 51.5
{1, 524288, 4, 1152, 3, 1, 10, 1},   // r4 train step, lone launch: one stream 142.5 -> 128.0 us, alone 141.0 -> 127.4
{1, 512, 1280, 10240, 1, 0, 14, 6},   // r4 train step, lone launch: one stream 45.6 -> 30.8 us, alone 45.2 -> 30.9
{1, 524288, 256, 128, 1, 0, 15, 1},   // r4 train step, lone launch: one stream 146.2 -> 141.2 us, alone 149.3 -> 141.9
{1, 524288, 128, 128, 1, 0, 15, 1},   // r4 train step, lone launch: one stream 76.0 -> 72.4 us, alone 75.8 -> 72.5
{1, 512, 1920, 11520, 3, 0, 10, 4},   // r4 train step, lone launch: one stream 131.2 -> 40.6 us, alone 130.8 -> 38.5
{1, 512, 1280, 3840, 1, 0, 8, 3},   // r4 train step, lone launch: one stream 23.9 -> 18.1 us, alone 23.8 -> 18.2
// -- round 5: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 16384, 256, 2304, 3, 3, 15, 1},   // r5 side-by-side: side 31.0 -> 24.5 us, alone 37.2 -> 40.1
{1, 65536, 128, 1152, 3, 3, 15, 1},   // r5 side-by-side: side 39.3 -> 33.8 us, alone 44.2 -> 40.2
// -- round 5: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 192, 10240, 1280, 1, 0, 15, 1},   // r5 side-by-side: side 14.7 -> 12.4 us, alone 22.6 -> 26.5
{1, 768, 3840, 1280, 1, 0, 15, 1},   // r5 side-by-side: side 16.2 -> 13.7 us, alone 22.4 -> 26.1
{1, 768, 10240, 1280, 1, 0, 15, 1},   // r5 side-by-side: side 41.4 -> 32.5 us, alone 47.1 -> 34.5
{1, 3072, 1920, 640, 1, 0, 15, 1},   // r5 side-by-side: side 16.4 -> 13.7 us, alone 22.6 -> 19.9
{1, 3072, 5120, 640, 1, 0, 15, 1},   // r5 side-by-side: side 44.1 -> 36.6 us, alone 50.6 -> 39.7
{1, 12288, 128, 1152, 3, 1, 10, 1},   // r5 side-by-side: side 15.4 -> 7.5 us, alone 29.7 -> 15.5
{1, 12288, 320, 1600, 1, 0, 15, 1},   // r5 side-by-side: side 22.7 -> 20.8 us, alone 23.7 -> 27.7
{1, 12288, 512, 512, 1, 0, 15, 1},   // r5 side-by-side: side 15.8 -> 14.3 us, alone 18.1 -> 18.0
{1, 12288, 1024, 512, 1, 0, 15, 1},   // r5 side-by-side: side 24.6 -> 22.0 us, alone 29.3 -> 23.5
{1, 12288, 2560, 320, 1, 0, 15, 1},   // r5 side-by-side: side 52.0 -> 46.6 us, alone 58.2 -> 49.4
{1, 49152, 512, 256, 1, 0, 15, 1},   // r5 side-by-side: side 32.7 -> 30.7 us, alone 36.1 -> 30.3
{1, 196608, 128, 1152, 3, 3, 15, 1},   // r5 side-by-side: side 116.0 -> 99.8 us, alone 128.2 -> 108.4
{1, 196608, 256, 128, 1, 0, 15, 1},   // r5 side-by-side: side 51.7 -> 49.6 us, alone 51.0 -> 44.4
{1, 196608, 256, 512, 1, 0, 15, 1},   // r5 side-by-side: side 108.6 -> 93.6 us, alone 125.4 -> 102.7
{1, 786432, 4, 1152, 3, 1, 10, 1},   // r5 side-by-side: side 205.7 -> 185.3 us, alone 214.6 -> 192.6
{1, 786432, 128, 64, 1, 0, 15, 1},   // r5 side-by-side: side 82.8 -> 79.0 us, alone 93.4 -> 85.4
{1, 786432, 128, 128, 1, 0, 15, 1},   // r5 side-by-side: side 104.5 -> 95.6 us, alone 119.8 -> 108.4
{1, 786432, 128, 256, 1, 0, 15, 1},   // r5 side-by-side: side 146.7 -> 137.1 us, alone 161.9 -> 148.8
// -- round 5: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 128, 2560, 11520, 3, 0, 14, 12},   // r5 side-by-side: side 36.2 -> 25.9 us, alone 35.8 -> 25.7
{1, 512, 5120, 1280, 1, 0, 14, 1},   // r5 side-by-side: side 22.1 -> 20.0 us, alone 22.0 -> 19.7
{1, 2048, 2560, 640, 1, 0, 17, 1},   // r5 side-by-side: side 17.8 -> 15.4 us, alone 18.1 -> 15.4
{1, 8192, 320, 1600, 1, 0, 16, 1},   // r5 side-by-side: side 19.9 -> 18.5 us, alone 19.6 -> 18.8
{1, 8192, 320, 2560, 1, 0, 16, 1},   // r5 side-by-side: side 26.5 -> 25.6 us, alone 26.8 -> 25.7
{1, 8192, 640, 2880, 3, 0, 10, 1},   // r5 side-by-side: side 49.9 -> 36.0 us, alone 52.0 -> 35.6
{1, 8192, 1280, 320, 1, 0, 17, 1},   // r5 side-by-side: side 17.7 -> 16.1 us, alone 18.3 -> 16.2
{1, 131072, 256, 512, 1, 0, 15, 1},   // r5 side-by-side: side 77.9 -> 66.1 us, alone 81.6 -> 66.6
{1, 524288, 12, 256, 1, 0, 3, 1},   // r5 side-by-side: side 54.0 -> 50.6 us, alone 54.0 -> 51.4
// -- round 5: shapes without a row so far (tools/tune_concurrent.py; variant 3 = stride 2)
{1, 128, 64, 1280, 1, 0, 7, 8},   // r5 side-by-side: side 3.1 -> 2.8 us, alone 6.9 -> 5.9
{1, 128, 1280, 1344, 1, 0, 7, 1},   // r5 side-by-side: side 5.1 -> 4.4 us, alone 9.9 -> 9.5
{1, 128, 3840, 1344, 1, 0, 7, 1},   // r5 side-by-side: side 8.8 -> 5.0 us, alone 16.1 -> 9.9
{1, 512, 1280, 1344, 1, 0, 7, 1},   // r5 side-by-side: side 9.4 -> 5.4 us, alone 15.3 -> 9.8
{1, 512, 3840, 1344, 1, 0, 14, 1},   // r5 side-by-side: side 13.0 -> 10.1 us, alone 21.2 -> 19.6
{1, 2048, 64, 640, 1, 0, 11, 1},   // r5 side-by-side: side 3.9 -> 2.7 us, alone 8.2 -> 6.1
{1, 2048, 640, 704, 1, 0, 11, 1},   // r5 side-by-side: side 5.1 -> 4.3 us, alone 10.2 -> 7.6
{1, 2048, 1920, 704, 1, 0, 15, 1},   // r5 side-by-side: side 10.4 -> 8.8 us, alone 15.3 -> 13.6
{1, 8192, 64, 320, 1, 0, 7, 1},   // r5 side-by-side: side 2.6 -> 2.2 us, alone 5.7 -> 4.9
{1, 8192, 960, 384, 1, 0, 15, 1},   // r5 side-by-side: side 12.6 -> 12.0 us, alone 17.8 -> 14.0
// -- round 6: every forward launch of the bench workloads is decided by a row (tests/test_parity_gpu.py::test_bench_workloads_have_tuned_rows).
// The shapes below had none: the side-by-side tuner (tools/tune_concurrent.py --workload slide / --lora, round 5) found no tile that beats the
// heuristic choice by its acceptance rule, so that choice is pinned -- a kernel change that moves one of them now needs a re-tune or an edit here.
{1, 524288, 256, 9216, 3, 0, 12, 1},   // slide: 2473.90 GFLOP, heuristic choice pinned (r6)
{1, 196608, 512, 4608, 3, 2, 12, 1},   // slide: 927.71 GFLOP, heuristic choice pinned (r6)
{1, 786432, 256, 2304, 3, 2, 12, 1},   // slide: 927.71 GFLOP, heuristic choice pinned (r6)
{1, 196608, 256, 4608, 3, 1, 12, 1},   // slide: 463.86 GFLOP, heuristic choice pinned (r6)
{1, 786432, 128, 2304, 3, 1, 12, 1},   // slide: 463.86 GFLOP, heuristic choice pinned (r6)
{1, 786432, 128, 1152, 3, 1, 12, 1},   // slide: 231.93 GFLOP, heuristic choice pinned (r6)
{1, 196608, 256, 2304, 3, 1, 12, 1},   // slide: 231.93 GFLOP, heuristic choice pinned (r6)
{1, 49152, 512, 4608, 3, 0, 12, 1},   // slide: 231.93 GFLOP, heuristic choice pinned (r6)
{1, 49152, 512, 4608, 3, 2, 12, 1},   // slide: 231.93 GFLOP, heuristic choice pinned (r6)
{1, 196608, 256, 1152, 3, 1, 12, 1},   // slide: 115.96 GFLOP, heuristic choice pinned (r6)
{1, 49152, 512, 2304, 3, 0, 12, 1},   // slide: 115.96 GFLOP, heuristic choice pinned (r6)
{1, 231, 24960, 768, 1, 0, 2, 1},   // slide: 8.86 GFLOP, heuristic choice pinned (r6)
{1, 12288, 320, 960, 1, 0, 2, 1},   // slide: 7.55 GFLOP, heuristic choice pinned (r6)
{1, 12288, 512, 576, 3, 0, 4, 1},   // slide: 7.25 GFLOP, heuristic choice pinned (r6)
{1, 3072, 640, 1280, 1, 0, 3, 1},   // slide: 5.03 GFLOP, heuristic choice pinned (r6)
{1, 12288, 320, 640, 1, 0, 2, 1},   // slide: 5.03 GFLOP, heuristic choice pinned (r6)
{1, 12288, 320, 576, 3, 0, 5, 1},   // slide: 4.53 GFLOP, heuristic choice pinned (r6)
{1, 12288, 512, 320, 1, 0, 2, 1},   // slide: 4.03 GFLOP, heuristic choice pinned (r6)
{1, 3072, 640, 960, 1, 0, 3, 1},   // slide: 3.77 GFLOP, heuristic choice pinned (r6)
{1, 192, 1280, 6400, 1, 0, 3, 9},   // slide: 3.15 GFLOP, heuristic choice pinned (r6)
{1, 12288, 320, 320, 1, 0, 2, 1},   // slide: 2.52 GFLOP, heuristic choice pinned (r6)
{1, 8192, 256, 512, 1, 0, 2, 1},   // slide: 2.15 GFLOP, heuristic choice pinned (r6)
{1, 8192, 320, 384, 1, 0, 2, 1},   // extract+lora: 2.01 GFLOP, heuristic choice pinned (r6)
{1, 3072, 512, 640, 1, 0, 3, 1},   // slide: 2.01 GFLOP, heuristic choice pinned (r6)
{1, 192, 3840, 1280, 1, 0, 3, 1},   // slide: 1.89 GFLOP, heuristic choice pinned (r6)
{1, 12288, 512, 128, 1, 0, 2, 1},   // slide: 1.61 GFLOP, heuristic choice pinned (r6)
{1, 3072, 640, 320, 1, 0, 3, 1},   // slide: 1.26 GFLOP, heuristic choice pinned (r6)
{1, 768, 1280, 640, 1, 0, 3, 1},   // slide: 1.26 GFLOP, heuristic choice pinned (r6)
{1, 12288, 128, 320, 1, 0, 3, 1},   // slide: 1.01 GFLOP, heuristic choice pinned (r6)
{1, 768, 512, 1280, 1, 0, 3, 5},   // slide: 1.01 GFLOP, heuristic choice pinned (r6)
{1, 3072, 128, 1152, 3, 1, 4, 4},   // slide: 0.91 GFLOP, heuristic choice pinned (r6)
{1, 154, 2560, 832, 1, 0, 3, 3},   // extract+lora: 0.66 GFLOP, heuristic choice pinned (r6)
{1, 2048, 256, 512, 1, 0, 3, 2},   // slide: 0.54 GFLOP, heuristic choice pinned (r6)
{1, 3072, 128, 640, 1, 0, 3, 2},   // slide: 0.50 GFLOP, heuristic choice pinned (r6)
{1, 3072, 512, 128, 1, 0, 3, 1},   // slide: 0.40 GFLOP, heuristic choice pinned (r6)
{1, 154, 1280, 832, 1, 0, 3, 3},   // extract+lora: 0.33 GFLOP, heuristic choice pinned (r6)
{1, 12288, 4, 2880, 3, 1, 5, 6},   // slide: 0.28 GFLOP, heuristic choice pinned (r6)
{1, 768, 128, 1280, 1, 0, 3, 5},   // slide: 0.25 GFLOP, heuristic choice pinned (r6)
{1, 768, 128, 1152, 3, 1, 4, 4},   // slide: 0.23 GFLOP, heuristic choice pinned (r6)
{1, 154, 640, 832, 1, 0, 3, 3},   // extract+lora: 0.16 GFLOP, heuristic choice pinned (r6)
{1, 3, 20160, 1280, 1, 0, 3, 1},   // slide: 0.15 GFLOP, heuristic choice pinned (r6)
{1, 512, 256, 512, 1, 0, 3, 2},   // slide: 0.13 GFLOP, heuristic choice pinned (r6)
{1, 768, 512, 128, 1, 0, 3, 1},   // slide: 0.10 GFLOP, heuristic choice pinned (r6)
{1, 512, 64, 1280, 1, 0, 3, 5},   // extract+lora: 0.08 GFLOP, heuristic choice pinned (r6)
{1, 154, 64, 768, 1, 0, 3, 3},   // extract+lora: 0.02 GFLOP, heuristic choice pinned (r6)
{1, 3, 1280, 1280, 1, 0, 3, 5},   // slide: 0.01 GFLOP, heuristic choice pinned (r6)
{1, 12288, 4, 64, 1, 0, 3, 1},   // slide: 0.01 GFLOP, heuristic choice pinned (r6)
{1, 3, 1280, 320, 1, 0, 3, 1},   // slide: 0.00 GFLOP, heuristic choice pinned (r6)
