// The kernel-selection values ("tuning keys") of the library, each written
// down once: X(name, default).  The table generates struct Knobs (all int),
// its constructor (every field read through UMAMD_TUNING="key=value,...",
// else the default), umamd::knobs() and um_set_tuning (knobs.hip).  Host code
// reads umamd::knobs().name where it decides, so a value set at run time
// holds from the next call on; a caller that sizes a buffer through a host
// query (um_colred_ws, um_bn_bwd_parts, um_bn_fwd_pool_parts_c,
// um_conv_wgrad_splits) must not change a key between the query and the launch.
#pragma once

#define UM_KNOBS(X)                                                                         \
  /* ---- implicit GEMM (igemm.hip): tiles and split-K ---- */                              \
  /* 64x64 tiles for deep layers: on/off, and below this many 128x128 tiles */              \
  X(small, 1)                                                                               \
  /* measured on MI355X (bench step, tools/sweep.sh): the deep layers' main */              \
  /* loops are load-latency bound (one double-buffered stage in flight per */               \
  /* block, ~1 us per k-step at 1 block per CU), so more, smaller and split */              \
  /* tiles help: 160/320/8/256 -> 600/1024/4/1024 took 578 -> 599 pairs/s */                \
  /* (split_below / split_target / split_minsteps / small_tiles) */                         \
  X(small_tiles, 1024)                                                                      \
  X(split_below, 600)                                                                       \
  X(split_target, 1024)                                                                     \
  X(split_minsteps, 4)                                                                      \
  /* the 8-wave LDS-DMA loop (glds bit 2) hides more of a 64x64-tile */                     \
  /* block's own latency: measured per conv (tools/ig_micro.sh), split only */              \
  /* below 256 tiles and to ~512 blocks -- 16x32x256->256 27 -> 24 us, */                   \
  /* 32x64x128->128 27 -> 19 us, 8x16x512->512 28 -> 25 us.  The register */                \
  /* path (reflect-fold data gradients, f32) keeps the thresholds above. */                 \
  X(glds_split_below, 256)                                                                  \
  X(glds_split_target, 512)                                                                 \
  /* halo kernel (halo_conv.hip) for "same" convs of at least this many tiles */            \
  X(halo, 1)                                                                                \
  X(halo_min_tiles, 256)                                                                    \
  /* widest output (columns) the halo kernel takes: 64 = one column block */                \
  /* (round 2); up to 192 adds 96/128-wide 3x3 blocks and column grids */                   \
  X(halo_max_nc, 192)                                                                       \
  /* 48-, 96- and 160-wide column tiles where they pad fewer columns */                     \
  X(odd_bn, 1)                                                                              \
  /* bit 0: 64-deep k-steps for the 64x64 tiles, bit 1: for the 128-row tiles */            \
  X(bk64, 3)                                                                                \
  /* bit 0: LDS-DMA main loop for the 64x64 tiles, bit 1: for the 128-row */                \
  /* tiles, bit 2: 8 waves per 64x64 tile.  Step sweep (tools/sweep.sh): */                 \
  /* 0 -> 653.6, 7 -> 654.8, 5 -> 661.3 pairs/s (the 128-row tiles keep the */              \
  /* register path: 3 LDS stages of 128-row tiles leave 1 block per CU) */                  \
  X(glds, 5)                                                                                \
  /* 6-stage LDS-DMA loop for 8-wave 64x64 grids of at most glds_deep_blocks */             \
  /* blocks (one 96 KB block per CU); 3 = off.  Step sweep: 3 -> 721, */                    \
  /* 6 -> 715 pairs/s (unsplit deep grids 713-717): five k-steps in flight */               \
  /* do not shorten the deep layers' k-loop, so latency is not its limit */                 \
  X(glds_deep, 3)                                                                           \
  X(glds_deep_blocks, 256)                                                                  \
  /* column-major tile order for weight-heavy GEMMs (0 off, 1 auto, 2 on): */               \
  /* per conv and per step within noise (714 vs 713 pairs/s), off */                        \
  X(xcd_col, 0)                                                                             \
  /* 8-channel operands: bit 0 packs 4 taps per 32-deep k-step, bit 1 also */               \
  /* routes them past the halo kernel.  First conv (7x7 s2, C8) 93 -> 51 us; */             \
  /* step 711 -> 715-716 pairs/s with 1 or 3 (the heads' halo path is as fast) */           \
  X(tappack, 1)                                                                             \
  /* the four parity classes of a stride-2 data gradient as one launch */                   \
  X(cls4, 1)                                                                                \
  /* the four parity classes of a stride-2 data gradient as one launch of */                \
  /* LDS-DMA tiles instead of 256-row register tiles (bit 0: NC a multiple */               \
  /* of 64 on 64x64 tiles: 64x128 C64 K128 59 -> 28 us, 32x64 C128 K256 */                  \
  /* 50 -> 24, 16x32 C256 K512 57 -> 28; bit 1: NC = 32 on 64x32 tiles with */              \
  /* 4 waves: 128x256 C32 K64 5x5 79 -> 63 us; MI355X, tools/gpu_s2_micro.sh) */            \
  X(cls_glds, 3)                                                                            \
  /* ---- reflect data gradient (conv.hip) ---- */                                          \
  /* reflect data gradient as a zero-pad transposed conv onto the padded */                 \
  /* input + a fold pass (0 off, 1 for dx wider than fold_split_nc, 2 all) */               \
  X(pad_dgrad, 1)                                                                           \
  /* reflect data gradients with more input channels than this run as one */                \
  /* fold pass, the others as a zero-pad pass + the border-list pass.  Per */               \
  /* conv (tools/conv_table.py): split form 256x512 C48 171 -> 117 us, */                   \
  /* C32 K8 125 -> 85; one pass stays ahead from C = 128 up (16x32 C640: */                 \
  /* 106 vs 140, 8x16 C512: 53 vs 79) */                                                    \
  X(fold_split_nc, 64)                                                                      \
  /* ---- halo conv (halo_conv.hip) ---- */                                                 \
  /* weight tap rows loaded two rows ahead (halo_conv.hip PF2) */                           \
  X(halo_pf2, 0)                                                                            \
  /* halo conv as persistent workgroups (resident count x this; 0 = one */                  \
  /* tile per workgroup) that prefetch the next tile's halo; halo_grid > 0 */               \
  /* caps the grid (tests: several tiles per workgroup on small images) */                  \
  X(halo_persist, 1)                                                                        \
  X(halo_grid, 0)                                                                           \
  /* 3x3 halo convs keep all their tap weights in LDS (per workgroup, for */                \
  /* all its tiles) when they need at most this many KB; 0 = stream rows */                 \
  X(halo_res_kb, 48)                                                                        \
  /* halo conv bf16 outputs through LDS as 16-byte rows (halo_conv.hip) */                  \
  X(halo_staged, 1)                                                                         \
  /* reflect fold of the split-form data gradient: a VALU pass over the */                  \
  /* border list (conv.hip reflect_border_kernel) instead of the GEMM */                    \
  /* (0 never, 1 K <= 8, 2 always) */                                                       \
  X(border_valu, 1)                                                                         \
  /* high-resolution 1x1 convs (M >= 16k, C <= 256, N <= 192) on the */                     \
  /* streaming kernel (stream1x1.hip) instead of 256-row GEMM tiles */                      \
  X(s1x1, 1)                                                                                \
  /* small-M 1x1 convs (stream1x1.hip s1x1_small_kernel, M < 16k pixels) */                 \
  X(s1x1_small, 1)                                                                          \
  /* ---- the other files; the measurements stand where the key is read ---- */             \
  /* all sources of a concat in one launch (decoder.hip; measured slower) */                \
  X(cat_fused, 0)                                                                           \
  /* merge backward: 2-4 sources on the loads-first instances (misc.hip) */                 \
  X(merge_ns, 1)                                                                            \
  /* column reduction (reduce.hip): one workgroup up to colred_single values, */            \
  /* else workgroups of at least colred_per values each */                                  \
  X(colred_single, 131072)                                                                  \
  X(colred_per, 16384)                                                                      \
  /* transposed-read weight gradient, pixels per k-step: 64 or 128, anything */             \
  /* else means 32 (wgrad_tr.hip) */                                                        \
  X(wtr_tbk, 32)                                                                            \
  /* the one-pass weight gradient of small 1x1 convs (conv.hip) */                          \
  X(w1x1, 1)                                                                                \
  /* split-K workspace for the border-list GEMM of a reflect fold (conv.hip) */             \
  X(border_split, 1)                                                                        \
  /* 1x1 conv + 2x upsampled add as a VALU kernel for C <= 16 (conv.hip) */                 \
  X(up2_valu, 1)                                                                            \
  /* generic weight gradient: target workgroups for the split count; 0 = */                 \
  /* from the chip (conv.hip generic_wgrad_splits) */                                       \
  X(wsplit_blocks, 0)                                                                       \
  /* slab reduction of R > 1 weight gradients through an LDS transpose */                   \
  X(wred_t, 1)                                                                              \
  /* cap of the rows per BN backward block (bn.hip bn_bwd_rows) */                          \
  X(bn_bwd_rows_max, 1024)                                                                  \
  /* 64-channel slices for the BN passes of small wide layers (bn.hip) */                   \
  X(bn_slice, 1)                                                                            \
  /* disparity head forward: 1 = the shift-load column kernel; dh_fwd128 = 0: */            \
  /* the k-split strips at C = 128 (disphead.hip) */                                        \
  X(dh_fwd, 0)                                                                              \
  X(dh_fwd128, 1)                                                                           \
  /* disparity head data gradient: 0 = unstaged 8-byte stores (disphead.hip) */             \
  X(dh_dgrad, 1)

namespace umamd {

struct Knobs {
#define UM_KNOB_FIELD(name, dflt) int name;
  UM_KNOBS(UM_KNOB_FIELD)
#undef UM_KNOB_FIELD
  Knobs();
};

Knobs& knobs();

}  // namespace umamd
