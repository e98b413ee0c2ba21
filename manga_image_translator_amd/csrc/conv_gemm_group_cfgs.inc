// conv_gemm_group_cfgs.inc — the tiles of conv_gemm_cfgs.inc that have a grouped twin (mit_conv_gemm_group: n convolutions that share
// everything but the image, as one grid).  G(name, family, the row's template arguments): conv_gemm.hip checks at compile time that the
// arguments are those of the row `name`, so a twin cannot drift from its tile.  The twins are kernels outside the tile table: a grouped
// launch is accounted under its tile's index.  Built for what the spatial convolutions of the 48px OCR backbone take (7x7 and 2x2 stem
// on the generic kernel; 3x3 stem and the four downsampling convs on the split tiles in GEMM mode 6 — always the buffer-load forms, a
// member whose offsets do not fit them sends the group to the member-by-member fallback — and on the fp32 MFMA tiles in mode 0).
G("128x128x16", generic, 128, 128, 16, 2, 2)
G("128x64x16", generic, 128, 64, 16, 2, 2)
G("fast128x128x16w4c", fast, 128, 128, 16, 1, 4, 4, 4)
G("fast128x64x16w5c", fast, 128, 64, 16, 2, 2, 5, 4)
G("fast64x64x16w8c", fast, 64, 64, 16, 2, 2, 8, 4)
G("split128x64x16p6u", split, 128, 64, 16, 2, 2, 3, 6, 2433)
G("split64x64x16p6u", split, 64, 64, 16, 2, 2, 4, 6, 2433)
G("split64x64x32p6u", split, 64, 64, 32, 2, 2, 3, 6, 2433)
G("split128x160x16p6u", split, 128, 160, 16, 4, 1, 2, 6, 2433)
G("split128x96x16p6u", split, 128, 96, 16, 4, 1, 3, 6, 2433)
