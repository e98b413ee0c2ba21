// conv_gemm_cfgs.inc — the tile configurations of mit_conv_gemm.  Refer to them BY NAME (mit_conv_gemm_config_name; conv_gemm_table.h's
// CFG): the index is only the position in this table.
// X(group, name, family, BM, BN, BK, remaining template arguments...)
//   group  : which conv_gemm_inst<group>.hip instantiates it (parallel compilation only)
//   family : the kernel and its launcher launch_<family> (TileFamily in conv_gemm_table.h):
//              generic  conv_gemm_kernel        launch_generic<BM,BN,BK,WAVES_M,WAVES_N>
//              fast     conv_gemm_fast_kernel   launch_fast<BM,BN,BK,WAVES_M,WAVES_N,MINW,VAR>                (needs fast_eligible())
//              gemv     conv_gemv_kernel        launch_gemv<ROWS_PER_ITERATION,NMAX,KVEC,LANES_PER_ROW>      (the BM/BN/BK columns hold its first three arguments)
//              split    conv_gemm_split_kernel  launch_split<BM,BN,BK,WAVES_M,WAVES_N,MINW,NPROD,VAR>         (needs MitConvGemm.w_split)
// A tile's traits (plane pairs, buffer loads, gemv lanes per row, its buffer-load twin) are read off these template arguments
// (CfgEntry); the tile choice names a tile through CFG("..."), which does not compile for a name that is not in this table.
// The table holds what pick_cfg() can return plus the reference forms the tests compare against.  The schedules that were measured and
// rejected, and the timing ablations, were removed; DESIGN.md and profiles/ keep their measurements, git history (e7f35b0) their code.
// ---- generic kernel (any Cin % 4 == 0, any number of taps, 64-bit offsets)
X(0, "128x128x16", generic, 128, 128, 16, 2, 2)  // general
X(0, "128x64x16", generic, 128, 64, 16, 2, 2)    // Cout <= 64
X(0, "128x32x16", generic, 128, 32, 16, 4, 1)    // Cout <= 32
// ---- fp32 MFMA fast kernel (GEMM mode 0, and every layer without split planes)
X(1, "fast128x128x16w4c", fast, 128, 128, 16, 1, 4, 4, 4)   // wide default: wave tile 128 x 32, <= 128 registers (4 workgroups per CU), gather offsets cached per tap
X(1, "fast128x64x16w5c", fast, 128, 64, 16, 2, 2, 5, 4)     // narrow default (N <= 64 or N % 128 <= 64): <= 96 registers
X(1, "fast192x64x16w4c", fast, 192, 64, 16, 2, 2, 4, 4)     // 128 < M <= 192 per batch entry (W-axis DFT fallback)
X(1, "fast64x64x16w8c", fast, 64, 64, 16, 2, 2, 8, 4)       // under-filled launches (decoder GEMMs)
X(1, "fast128x32x16w4c", fast, 128, 32, 16, 4, 1, 4, 4)     // N <= 32 (ESRGAN's growth-32 convolutions)
// ---- N <= 4 on the VALU (conv_gemv_kernel)
X(0, "gemv16", gemv, 8, 4, 4, 16)   // Cin % 64 == 0: 16 lanes per output pixel
X(0, "gemv4", gemv, 8, 4, 4, 4)     // Cin % 16 == 0: 4 lanes per output pixel
X(0, "gemv16n1", gemv, 8, 1, 4, 16) // N == 1 forms of the two
X(0, "gemv4n1", gemv, 4, 1, 4, 4)
// ---- split-bf16 tiles (GEMM mode 6 | 9): fp32 as three bf16 planes, NPROD plane pairs on the bf16 MFMA.  "o" / "m": the staging of the
// next K-tile placed step by step behind the MFMAs (VAR 1 + 128), "o" also with the fragment reads in consumption order (+ 256)
X(4, "split128x128x16p6o", split, 128, 128, 16, 2, 2, 3, 6, 385)  // the shipped wide tile
X(4, "split128x128x16p9m", split, 128, 128, 16, 2, 2, 3, 9, 129)
X(4, "split128x64x16p6o", split, 128, 64, 16, 2, 2, 3, 6, 385)    // the shipped narrow tile
X(3, "split128x64x16p9", split, 128, 64, 16, 2, 2, 2, 9, 0)
X(3, "split64x64x16p6o", split, 64, 64, 16, 2, 2, 4, 6, 385)      // under-filled launches (same arithmetic per output element as the large tiles)
X(3, "split64x64x16p9m", split, 64, 64, 16, 2, 2, 4, 9, 129)
X(3, "split64x64x32p6o", split, 64, 64, 32, 2, 2, 3, 6, 385)      // ... with two MFMA steps per barrier for latency-bound launches
X(3, "split64x64x32p9m", split, 64, 64, 32, 2, 2, 3, 9, 129)
X(3, "split128x32x16p6o", split, 128, 32, 16, 4, 1, 4, 6, 385)    // N <= 32
X(3, "split128x32x16p9m", split, 128, 32, 16, 4, 1, 4, 9, 129)
X(3, "split128x160x16p6o", split, 128, 160, 16, 4, 1, 2, 6, 385)   // N = 160 / 320 / 640 / 1280 without padded columns: wave tile 32 x 160
X(3, "split128x96x16p6o", split, 128, 96, 16, 4, 1, 3, 6, 385)     // N = 80 (ConvNeXt stage-1 pw2): 96 computed columns instead of 128
X(3, "split128x192x16p6o", split, 128, 192, 16, 4, 1, 2, 6, 385)   // N = 192 / 384 (LaMa spectral convs): wave tile 32 x 192
// ---- "u": the shipped p6 tiles with their operand loads through buffer instructions (VAR + 2048, round 6): descriptor + 32-bit byte
// offset per lane, rows that contribute zeros answered by the range check — 58 instead of 77 VALU instructions per K-tile beside the 24
// MFMAs, 1.03-1.06x on every shape (profiles/r10s_split_check_buffer_loads.log), same bits.  pick_cfg takes them whenever every A and W
// byte offset is below 2^31 (buf_eligible), else the "o" twin.
X(2, "split128x128x16p6u", split, 128, 128, 16, 2, 2, 3, 6, 2433)
X(2, "split128x64x16p6u", split, 128, 64, 16, 2, 2, 3, 6, 2433)
X(2, "split64x64x16p6u", split, 64, 64, 16, 2, 2, 4, 6, 2433)
X(2, "split64x64x32p6u", split, 64, 64, 32, 2, 2, 3, 6, 2433)
X(5, "split128x32x16p6u", split, 128, 32, 16, 4, 1, 4, 6, 2433)
X(5, "split128x160x16p6u", split, 128, 160, 16, 4, 1, 2, 6, 2433)
X(5, "split128x96x16p6u", split, 128, 96, 16, 4, 1, 3, 6, 2433)
X(5, "split128x192x16p6u", split, 128, 192, 16, 4, 1, 2, 6, 2433)
// reference forms for the tests: the plain (unpipelined) schedule of the same arithmetic, and the 3-pair rung of the accuracy ladder
X(3, "split128x128x16p6", split, 128, 128, 16, 2, 2, 2, 6, 0)
X(3, "split128x128x16p9", split, 128, 128, 16, 2, 2, 2, 9, 0)
X(3, "split128x128x16p3", split, 128, 128, 16, 2, 2, 2, 3, 0)     // 16-bit-significand products (tests only)
X(3, "split128x64x16p6", split, 128, 64, 16, 2, 2, 2, 6, 0)
// ---- "p1" (MitConvGemm.nprod = 1, conv_gemm_split.h): ONE product of the bf16 roundings of both operands, fp32 accumulation — the opt-in
// bf16 precision (LaMa's precision="bf16"), never a GEMM mode.  K-tile 32; "o" / "u" as above.  All of them give the same bits.
X(6, "split128x128x32p1o", split, 128, 128, 32, 2, 2, 3, 1, 385)   // wide
X(6, "split128x128x32p1u", split, 128, 128, 32, 2, 2, 3, 1, 2433)
X(6, "split128x64x32p1o", split, 128, 64, 32, 2, 2, 3, 1, 385)     // narrow (N <= 64 or N % 128 <= 64)
X(6, "split128x64x32p1u", split, 128, 64, 32, 2, 2, 3, 1, 2433)
X(6, "split128x192x32p1o", split, 128, 192, 32, 4, 1, 2, 1, 385)   // N = 192 / 384 (LaMa spectral convs): wave tile 32 x 192
X(6, "split128x192x32p1u", split, 128, 192, 32, 4, 1, 2, 1, 2433)
X(6, "split64x64x32p1o", split, 64, 64, 32, 2, 2, 4, 1, 385)       // under-filled launches
X(6, "split64x64x32p1u", split, 64, 64, 32, 2, 2, 4, 1, 2433)
X(6, "split64x64x16p1o", split, 64, 64, 16, 2, 2, 4, 1, 385)       // Cin % 32 != 0 (a K-tile must lie inside one tap)
X(6, "split64x64x16p1u", split, 64, 64, 16, 2, 2, 4, 1, 2433)
