/*
 * stainx_hip.h -- C ABI of libstainx_hip.so, the MI355X (gfx950) stain-normalisation library.
 *
 * This is the drop-in boundary for the hot path of rendeirolab/stainx: the four functions its
 * pybind11 extension `stainx_cuda_torch` exports (src/stainx_cuda_torch/csrc/bindings.cpp:31-34)
 * plus the fit-time statistics the reference computes with its torch backend
 * (src/stainx/backends/torch_backend.py:143-179, 308-323, 463-519).
 *
 * Conventions
 *  - plain C: pointers, sizes, enums.  No torch / ATen types.
 *  - every pointer named *_dev is DEVICE memory owned by the caller (torch's caching allocator in the
 *    Python host); the library never allocates, frees or retains pointers.
 *  - `stream` is a hipStream_t passed as void*; every entry point only enqueues work on it and never
 *    synchronises the host (stainx's Macenko/HM natives are asynchronous too: macenko.cu:102).
 *  - images are dense NCHW (HM: optionally NHWC) with C == 3, element type `dtype`.
 *  - return value: SX_OK or an sx_status error; sx_last_error_string() describes the last error of
 *    the calling thread.  Nothing throws or aborts.
 *  - `workspace_dev` must hold at least sx_*_workspace_bytes() bytes, 256-byte aligned.  Its contents
 *    need no initialisation and are dead after the call (except for sx_macenko_tile_params()).
 */
#ifndef STAINX_HIP_H
#define STAINX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SX_ABI_VERSION 1

typedef enum { SX_U8 = 0, SX_F16 = 1, SX_BF16 = 2, SX_F32 = 3, SX_F64 = 4 } sx_dtype;

typedef enum {
    SX_OK = 0,
    SX_ERR_BAD_ARG = 1,    /* null pointer, non-positive size, C != 3 ... (reference: TORCH_CHECK -> RuntimeError) */
    SX_ERR_DTYPE = 2,      /* unsupported element type */
    SX_ERR_WORKSPACE = 3,  /* workspace too small or misaligned */
    SX_ERR_LAUNCH = 4      /* hipGetLastError() after a launch (reference: macenko.cu:125-126) */
} sx_status;

/* flags for sx_macenko_transform: the six public bits */
#define SX_MACENKO_NORMALIZE_0_1 1u /* fuse `result / 255.0` (normalizers/_template.py:111-112); u8 input -> f32 output */
#define SX_MACENKO_CHANNELS_LAST 2u /* images and output are (N,H,W,3) (decoder / PIL layout) instead of (N,3,H,W); an extension: the
                                      reference takes NCHW only and callers permute + copy first */
#define SX_MACENKO_SAMPLED 4u       /* an APPROXIMATION (not a parity path, not the reference's precision="fast"): the percentiles of a 4096-pixel
                                      sample of each tile stand in for the exact ones -- moments pass, one per-tile stage, reconstruct.  Mean
                                      error ~0.5, worst ~5 grey levels on H&E tiles.  Macenko(precision="sampled") in the Python host; the
                                      reference's precision="fast" (fp16 tensors, exact percentiles, MAE ~0.05) is served by the exact path. */
#define SX_MACENKO_CLASSIC 16u       /* the four-pass form of the transform even where the two-pass form would be chosen (same bits; callers whose
                                       batches hold tiles the two-pass form cannot speculate on: see sx_macenko_telemetry_offset) */
#define SX_MACENKO_OUT_BF16 32u      /* uint8 input only: the result is written as bfloat16 -- bit for bit `transform(x).to(bfloat16)`, with
                                       SX_MACENKO_NORMALIZE_0_1 `transform(x, normalize_to_0_1).to(bfloat16)` -- so a uint8 tile from the decoder
                                       becomes a model's bf16 input with 3 bytes read and 6 written per pixel (an extension: SURVEY.md 8f-2) */
#define SX_MACENKO_OUT_F16 64u       /* the same with float16 */

/* Diagnostic builds only (-DSX_DIAG: stainx_amd/_lib/libstainx_diag.so, built next to the product by __graft_entry__.build(); the product
   library refuses these bits with SX_ERR_BAD_ARG).  Tests force the rare paths with them; two measured-and-slower forms of the transform
   live there as design studies (DESIGN.md sections 4c, 4e). */
#ifdef SX_DIAG
#define SX_MACENKO_NO_TIE_SHORTCUT 8u /* do not resolve a bracket that closed on one key from its counts (forces the slow exact paths) */
#define SX_MACENKO_SPEC_FAIL 128u    /* the two-pass form treats every speculation as failed (forces its slow exact path) */
#define SX_MACENKO_TWO_PASS 256u     /* the two-pass form wherever it can run (by default only where it is the faster one) */
#define SX_MACENKO_FUSE 512u         /* the two-pass form with its last three launches as ONE launch with tile-level dependencies (planar float32 tiles of
                                       128x128 ... 512x512; same bits; slower: DESIGN.md 4c) */
#define SX_MACENKO_RESIDENT 1024u    /* the tile-resident form: one launch, a tile's pixels kept on chip as 8-bit codes (same bits; slower: DESIGN.md 4e) */
#define SX_MACENKO_NO_CODES 2048u    /* the four passes over float32 tiles read the float pixels in every pass (by default the first pass leaves 8-bit codes
                                       of the tiles that consist of grey levels and the later passes read those: same bits) */
#endif

int sx_version(void);
const char* sx_last_error_string(void);

/* ---------------------------------------------------------------- Macenko ------------------------
 * Replaces stainx_cuda_torch.macenko (bindings.cpp:33; src/stainx_cuda_torch/csrc/macenko.cu:67-266)
 * with the numerics of MacenkoTorch.transform (torch_backend.py:521-560).
 *   images_dev        (N,3,H,W) `dtype`; u8 is [0,255], floats are taken as [0,1] as is
 *   out_dev           (N,3,H,W) same dtype (f32 when dtype==SX_U8 and SX_MACENKO_NORMALIZE_0_1; bf16 / f16 when dtype==SX_U8 and
 *                     SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16); (N,H,W,3) in and out with SX_MACENKO_CHANNELS_LAST
 *   stain_matrix_dev  6 floats, row-major (3,2)      target_max_conc_dev  2 floats
 */
size_t sx_macenko_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
/* sx_macenko_workspace_bytes() serves ANY sx_macenko_* call on such a batch.  What ONE sx_macenko_transform call with these
 * arguments needs is a prefix of it and can be much less: the call checks its workspace against THIS size (narrow pixels and
 * small batches take the four-pass form and none of the two-pass areas; the fused launch does not need the four-launch form's
 * candidate arrays).  sx_macenko_fit and the sx_macenko_dfit_* and sx_macenko_pfit_* steps need the size of a call with SX_MACENKO_CLASSIC. */
size_t sx_macenko_workspace_bytes_for(int dtype, int64_t n_tiles, int64_t height, int64_t width, unsigned flags);

int sx_macenko_transform(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                         int64_t width, const float* stain_matrix_dev, const float* target_max_conc_dev,
                         unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Byte offset, inside the workspace, of a uint32 RUNNING count of per-tile selections that left the speculative path of the
 * two-pass form (tiles without tissue, tiles without a stable stain plane ...: each costs a whole-tile exact select, ~0.1-0.5 ms).
 * The library only ever adds to it (its value in a fresh workspace is whatever the memory held): a host reads it back
 * asynchronously, takes the difference to what it read before, and passes SX_MACENKO_CLASSIC for data that makes it grow -- the
 * four-pass form has no such cliff.  (A count per call would be reset by the next call's first kernel before a host that lets
 * its calls queue up could read it.) */
size_t sx_macenko_telemetry_offset(void);

/* 1 if sx_macenko_transform takes its two-pass form for such a call (element type, batch, tile size, flags), 0 for the four-pass
 * form: a host only needs to watch the telemetry word after calls of the first kind. */
int sx_macenko_takes_two_pass(int dtype, int64_t n_tiles, int64_t height, int64_t width, unsigned flags);
/* The same in full: 0 four passes, 1 two-pass form as four launches, 2 two-pass form with pass A, the per-tile stages and the
 * reconstruct pass in one launch (only with SX_MACENKO_FUSE; falls back to 0 at call time when a pointer is not 16-byte aligned). */
int sx_macenko_form(int dtype, int64_t n_tiles, int64_t height, int64_t width, unsigned flags);

/* Replaces MacenkoTorch.compute_reference_stain_matrix_torch (torch_backend.py:463-519): one stain
 * estimate pooled over all n_tiles*H*W pixels, no "<3 kept pixels" fallback.
 *   he_out_dev 6 floats (3,2) row-major;  max_c_out_dev 2 floats */
int sx_macenko_fit(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                   float* he_out_dev, float* max_c_out_dev, void* workspace_dev, size_t workspace_bytes,
                   void* stream);

/* Stain augmentation (Tellez et al.; torchstain's MacenkoAugmentor, HistomicsTK's rgb_perturb_stain_concentration): every tile is
 * split into its H and E concentrations C = pinv(HE_source) OD in its own stain basis (the transform's per-tile estimate, exact
 * percentiles), the concentrations are scaled and shifted by the tile's own factors, and the tile is rebuilt.  An extension: the
 * reference has no counterpart.
 *   alpha_dev, beta_dev   n_tiles x 2 floats each, (H, E) per tile, DEVICE memory read by the last kernel of the call (a captured
 *                         graph replayed after new values are written into the same buffers uses the new values)
 *   own basis             stain_matrix_dev == target_max_conc_dev == NULL:
 *                           C' = alpha * C + beta,                       OD' = HE_source C'
 *   normalise and jitter  both given (a fitted reference, as for sx_macenko_transform):
 *                           C' = alpha * (C * target_max_conc / maxC) + beta,   OD' = stain_matrix C'
 *                         then, as the transform (the reference's Io = 240): out = clamp(240 exp(-OD'), 0, 255), cast to the output
 *                         type.  Exactly one of the two pointers NULL is SX_ERR_BAD_ARG.
 * Images, output and its element type follow sx_macenko_transform's rules; flags: SX_MACENKO_NORMALIZE_0_1, SX_MACENKO_CHANNELS_LAST,
 * SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16 (uint8 input), and SX_MACENKO_CLASSIC (a no-op: augmentation always takes the four-pass
 * form); any other bit, SX_MACENKO_SAMPLED included, is SX_ERR_BAD_ARG.  alpha = 1, beta = 0 in normalise mode gives the bits of
 * sx_macenko_transform(..., SX_MACENKO_CLASSIC).  The workspace needs sx_macenko_workspace_bytes_for(dtype, n_tiles, height, width,
 * SX_MACENKO_CLASSIC) bytes.  Own-basis mode skips the concentration percentiles (three passes over the input instead of four):
 * sx_macenko_tile_params after it reports the plane, the angles and HE_source, but no maxC (those two floats are stale). */
int sx_macenko_augment(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                       const float* alpha_dev, const float* beta_dev,
                       const float* stain_matrix_dev, const float* target_max_conc_dev,
                       unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Stain separation (torchstain's normalize(..., stains=True), HistomicsTK's color_deconvolution, tiatoolbox's get_concentrations): every
 * tile's H and E concentrations C = pinv(HE_source) OD, with the transform's per-tile estimate (exact percentiles), as images of one
 * stain each and / or as concentration maps.
 *   own basis    stain_matrix_dev == target_max_conc_dev == NULL:  C' = C,                        images built with the tile's HE_source
 *   normalised   both given (a fitted reference):                  C' = C * target_max_conc / maxC, images built with stain_matrix
 *                Exactly one of the two pointers NULL is SX_ERR_BAD_ARG.
 *   H = clamp(240 exp(-basis[:,0] C'_H), 0, 255), E likewise with column 1 (torchstain's (H, E) with Io = 240), cast as the transform
 *   casts: the input dtype; float32 /255 with SX_MACENKO_NORMALIZE_0_1 on uint8, the /255 fused on float input; bf16 / f16 with
 *   SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16 on uint8.  A tile whose maxC is 0 gets an infinite scale (as the transform); the other
 *   stain's image and concentrations are not affected by it.
 * Outputs, each may be NULL; at least one of stains_out_dev and conc_out_dev is required (SX_ERR_BAD_ARG otherwise):
 *   stains_out_dev      (2, N, 3, H, W) of the image element: the H images, then the E images; (2, N, H, W, 3) with SX_MACENKO_CHANNELS_LAST
 *   conc_out_dev        (N, 2, H, W) float32, C' (H, E); (N, H, W, 2) with SX_MACENKO_CHANNELS_LAST
 *   tile_he_out_dev     N x 6 floats, HE_source (3, 2) row-major
 *   tile_max_c_out_dev  N x 2 floats, maxC.  Free in normalised mode; in own-basis mode it adds the concentration bracket pass and the
 *                       scale stage that own basis otherwise skips.
 * Flags: SX_MACENKO_NORMALIZE_0_1, SX_MACENKO_CHANNELS_LAST, SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16 (uint8 input), SX_MACENKO_CLASSIC
 * (a no-op: separation always takes the four-pass estimate); any other bit, SX_MACENKO_SAMPLED included, is SX_ERR_BAD_ARG.  The workspace
 * needs sx_macenko_workspace_bytes_for(dtype, n_tiles, height, width, SX_MACENKO_CLASSIC) bytes.  The H image is the bits of
 * sx_macenko_augment(alpha = (1, 0), beta = (0, 0)) with the same reference or none, the E image those of alpha = (0, 1), wherever the
 * other stain's scale is finite.  sx_macenko_tile_params after it reports the estimate (own basis without tile_max_c_out_dev: no maxC). */
int sx_macenko_separate(const void* images_dev, void* stains_out_dev, float* conc_out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                        const float* stain_matrix_dev, const float* target_max_conc_dev, float* tile_he_out_dev, float* tile_max_c_out_dev,
                        unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Slide-level use (torchstain's fit-the-source-elsewhere, tiatoolbox's and HistomicsTK's given stain matrices): estimate the source basis
 * in one call, apply a GIVEN basis in another.  An extension: the reference estimates per tile inside every transform.
 *
 * sx_macenko_estimate: the transform's per-tile estimate (four passes, exact percentiles) and nothing else -- no output pass.
 *   tile_he_out_dev      N x 6 floats, HE_source (3, 2) row-major
 *   tile_max_c_out_dev   N x 2 floats, maxC
 *   tile_tissue_out_dev  N floats, the pixels the optical-density filter kept (the tile's tissue); may be NULL
 * They are the bits sx_macenko_tile_params reports (HE_source, maxC, n_selected) after sx_macenko_transform(..., SX_MACENKO_CLASSIC) of
 * the same batch.  Flags: SX_MACENKO_CHANNELS_LAST, SX_MACENKO_CLASSIC (a no-op); any other bit is SX_ERR_BAD_ARG.  The workspace needs
 * sx_macenko_workspace_bytes_for(dtype, n_tiles, height, width, SX_MACENKO_CLASSIC) bytes.  (One basis pooled over a batch: sx_macenko_fit.) */
int sx_macenko_estimate(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                        float* tile_he_out_dev, float* tile_max_c_out_dev, float* tile_tissue_out_dev,
                        unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);

/* sx_macenko_apply: normalise (and optionally jitter) every tile with a GIVEN source basis -- ONE kernel launch on `stream`, nothing
 * else enqueued, no workspace: a pixel is read, a pixel is written.
 *   source_he_dev        n_sources x 6 floats, HE_source (3, 2) row-major
 *   source_max_c_dev     n_sources x 2 floats, maxC; not read in own-basis mode, where it may be NULL
 *   n_sources            1 (one basis for the whole batch) or n_tiles (row t serves tile t)
 *   alpha_dev, beta_dev  n_tiles x 2 floats each, (H, E) per tile, both or neither (neither: alpha = 1, beta = 0)
 *   normalise            stain_matrix_dev and target_max_conc_dev given (a fitted reference, as for sx_macenko_transform):
 *                          C = pinv(source_he) OD,  C' = alpha * (C * target_max_conc / source_max_c) + beta,  OD' = stain_matrix C'
 *   own basis            both NULL, alpha and beta required:  C' = alpha * C + beta,  OD' = source_he C'
 *                        then, as the transform: out = clamp(240 exp(-OD'), 0, 255), cast to the output type.
 * Exactly one pointer of a pair NULL, n_sources other than 1 or n_tiles, own basis without factors, source_max_c_dev NULL in normalise
 * mode: SX_ERR_BAD_ARG, before anything is enqueued.  The source, the factors and the reference are DEVICE memory read by the kernel (a
 * captured graph replayed after new values were written into the same buffers uses the new values).  Images, output and its element
 * type follow sx_macenko_transform's rules; flags: SX_MACENKO_NORMALIZE_0_1, SX_MACENKO_CHANNELS_LAST, SX_MACENKO_OUT_BF16 /
 * SX_MACENKO_OUT_F16 (uint8 input) and SX_MACENKO_CLASSIC (a no-op); any other bit, SX_MACENKO_SAMPLED included, is SX_ERR_BAD_ARG.
 * The pseudo-inverse is a function of the six given floats (fp64, the rank rule of lstsq(rcond=None): a rank-1 basis drops its second
 * singular value), the scale a float32 division, so a tile's own estimate fed back -- sx_macenko_estimate's outputs, n_sources =
 * n_tiles -- gives the bits of sx_macenko_transform(..., SX_MACENKO_CLASSIC) without factors and of sx_macenko_augment with them,
 * wherever the tile's maxC is finite and non-zero.
 * Verified parameter domain (tests/_param_sweep.py): the parity bound of 2.55e-2 on the 0-255 scale against the float64
 * arithmetic is verified for finite bases with cond(HE) = sigma_max / sigma_min <= 25 (a stain angle of about 0.08 rad; the estimates of
 * H&E tiles measured lie at 3.3 ... 11.4) whose column sums are positive, a finite positive maxC with target_max_conc / maxC / |column|
 * in [0.05, 2.5], and finite factors with alpha in [-1.2, 1.2] and |beta| <= 3.  The float32 fold itself leaves the quarter of the bound
 * it is allowed near cond 100 and the bound near cond 500: a narrower angle is a caller's error, not caught here.  Outside the domain
 * every output element is still finite and inside the output range, and a tile's result depends on its own row alone. */
int sx_macenko_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                     const float* source_he_dev, const float* source_max_c_dev, int64_t n_sources,
                     const float* alpha_dev, const float* beta_dev,
                     const float* stain_matrix_dev, const float* target_max_conc_dev,
                     unsigned flags, void* stream);

/* Tissue masks: the three calls above with an explicit mask -- the Macenko estimate taken over the masked-in pixels only, the masked-out
 * pixels copied.  An extension (the reference's only notion of tissue is the optical-density filter, which protects the stain vectors
 * but not the concentration percentiles: on a tile that is mostly glass maxC comes out too small and the tissue is over-darkened).
 *   mask_dev   (N, H, W), one byte per pixel, non-zero = in: what sx_tissue_mask writes.  Explicit masks only: a caller that wants the
 *              luminosity rule runs sx_tissue_mask first.  NULL is SX_ERR_BAD_ARG.
 * The contract: masked Macenko is the reference's algorithm run on the masked-in pixels of a group (a tile, or the pooled batch) --
 * the optical-density filter, the "fewer than 3 kept -> every pixel" fallback (per tile only; "every pixel" = every masked-in pixel), the
 * covariance, plane, angle percentiles, stain vectors and the concentration percentiles, with nearest ranks over the masked-in set, not
 * over H*W.  A masked-in pixel of the output gets exactly the arithmetic of the unmasked reconstruct pass with its tile's estimate.  A
 * masked-out pixel is COPIED: its input level on the 0-255 scale (uint8: the byte; floats: x * 255 formed in float32) goes through the
 * output path of the tissue pixels -- clamp to [0, 255], cast to the output element, the optional / 255 -- so uint8 in, uint8 out is
 * byte-identical there.  The values under masked-out pixels do not matter at all, NaN and Inf included (every use is a select).  The
 * edge is hard.  A group WITHOUT an estimate -- per tile: fewer than 3 masked-in pixels; pooled, where the reference's fit has no
 * fallback: fewer than 3 pixels both masked-in and kept by the filter -- has NaN HE and maxC rows and a kept count of 0;
 * sx_macenko_transform_masked copies such a tile through (every pixel by the background rule), sx_macenko_apply_masked copies a tile
 * whose source row holds a NaN (as sx_reinhard_apply_stats_masked does); the unmasked sx_macenko_apply is not changed.
 * With every mask byte set the three calls give the BITS of sx_macenko_estimate / sx_macenko_fit, of sx_macenko_transform(...,
 * SX_MACENKO_CLASSIC) and of sx_macenko_apply (same grids, same reduction order) wherever those have an estimate.
 * They always run the four-pass form over planar (N,3,H,W) tiles, read the float pixels in every pass (no 8-bit codes), make no host
 * synchronisation and are capturable.  The mask is read in packs as wide as the pixel packs (16 / 8 / 4 bytes for uint8 / 16-bit /
 * float32 pixels) where the image pointers, the tile size AND the mask pointer allow it, one byte at a time otherwise; the mask
 * pointer's alignment is independent of the images'.
 * Flags: SX_MACENKO_NORMALIZE_0_1, SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16 (uint8 input) -- transform and apply --, SX_MACENKO_CLASSIC
 * (a no-op, all three).  SX_MACENKO_SAMPLED, SX_MACENKO_CHANNELS_LAST and any other bit are SX_ERR_BAD_ARG before anything is enqueued,
 * as are the argument errors of the unmasked calls.  Workspace (estimate, transform): sx_macenko_workspace_bytes_for(dtype, n_tiles,
 * height, width, SX_MACENKO_CLASSIC) bytes -- the masked forms keep their one extra datum, the work items' masked-in counts, in an area
 * that is free during the moments pass.
 *
 * sx_macenko_estimate_masked: pooled == 0: n_tiles rows, the transform's per-tile estimate over the masked-in pixels; pooled != 0: ONE
 * row over the masked-in pixels of the whole batch (sx_macenko_fit's path, without a fallback).
 *   he_out_dev, max_c_out_dev   rows x 6 / rows x 2 floats
 *   kept_out_dev                rows floats: the pixels of the selection set (masked-in and kept by the filter; the masked-in pixels of a
 *                               tile that took them all; 0 without an estimate); may be NULL
 *   mask_counts_out_dev         rows x uint64: the masked-in pixels of the group, exact; may be NULL */
int sx_macenko_estimate_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, const unsigned char* mask_dev, int pooled,
                               float* he_out_dev, float* max_c_out_dev, float* kept_out_dev, unsigned long long* mask_counts_out_dev,
                               unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);
/* sx_macenko_transform_masked: the masked per-tile estimate followed by a masked reconstruct pass (sx_macenko_transform's other arguments). */
int sx_macenko_transform_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, const unsigned char* mask_dev,
                                const float* stain_matrix_dev, const float* target_max_conc_dev, unsigned flags, void* workspace_dev, size_t workspace_bytes,
                                void* stream);
/* sx_macenko_apply_masked: sx_macenko_apply (all its modes: n_sources 1 or n_tiles, factors or none, normalise or own basis) under a mask --
 * ONE kernel launch on `stream`, nothing else enqueued, no workspace; source, factors, reference and mask are device memory read by the
 * kernel.  transform_masked(x, m) has the bits of apply_masked(x, estimate_masked(x, m), m). */
int sx_macenko_apply_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                            const float* source_he_dev, const float* source_max_c_dev, int64_t n_sources,
                            const float* alpha_dev, const float* beta_dev,
                            const float* stain_matrix_dev, const float* target_max_conc_dev,
                            const unsigned char* mask_dev, unsigned flags, void* stream);

/* ---- separation and augmentation: given source basis, tissue masks ----
 * sx_macenko_separate_apply: sx_macenko_separate's streaming pass with a GIVEN source basis -- ONE kernel launch on `stream`, nothing else
 * enqueued, no workspace, no estimate; a pixel is read once.  Outputs and flags are sx_macenko_separate's (either output may be NULL, not
 * both), the source arguments sx_macenko_apply's: n_sources is 1 (one basis for the batch) or n_tiles; source_max_c_dev may be NULL in own
 * basis (stain_matrix_dev and target_max_conc_dev both NULL: images built with the given HE, concentrations unscaled); source, reference
 * and mask are device memory read by the kernel (a captured call replayed after new values were copied in uses them).
 * separate_apply(x, estimate(x)) with n_tiles rows has the bits of sx_macenko_separate(x) wherever the tile's maxC is finite and
 * non-zero; with one row the result does not depend on n_sources.  NaN source rows are not special-cased (as in sx_macenko_apply). */
int sx_macenko_separate_apply(const void* images_dev, void* stains_out_dev, float* conc_out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                              const float* source_he_dev, const float* source_max_c_dev, int64_t n_sources,
                              const float* stain_matrix_dev, const float* target_max_conc_dev, unsigned flags, void* stream);
/* sx_macenko_separate_apply_masked: the same under a mask (N, H, W), one byte per pixel, planar tiles only (SX_MACENKO_CHANNELS_LAST is
 * refused, a NULL mask is an error).  A masked-out pixel holds no stain: both concentrations are +0.0f, both stain images the level of
 * zero concentration, 240, cast (and / 255) as a tissue pixel's level is.  Values under masked-out pixels are never used (NaN and Inf
 * included).  A tile whose source row holds a NaN -- in normalised mode its maxC row counts too -- is masked-out entirely.  With a mask of
 * all ones: the bits of sx_macenko_separate_apply. */
int sx_macenko_separate_apply_masked(const void* images_dev, void* stains_out_dev, float* conc_out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                                     const float* source_he_dev, const float* source_max_c_dev, int64_t n_sources,
                                     const float* stain_matrix_dev, const float* target_max_conc_dev,
                                     const unsigned char* mask_dev, unsigned flags, void* stream);
/* sx_macenko_separate_masked: sx_macenko_separate's arguments plus the mask: the masked per-tile estimate (sx_macenko_estimate_masked's
 * launches; own basis without tile_max_c_out_dev stops after the stain stage), then the masked separation pass over its rows -- the bits
 * of sx_macenko_estimate_masked followed by sx_macenko_separate_apply_masked.  A tile without an estimate (fewer than 3 masked-in pixels)
 * has NaN tile_he / tile_max_c rows and comes out entirely as background.  Workspace: sx_macenko_workspace_bytes_for(..., SX_MACENKO_CLASSIC). */
int sx_macenko_separate_masked(const void* images_dev, void* stains_out_dev, float* conc_out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                               const unsigned char* mask_dev, const float* stain_matrix_dev, const float* target_max_conc_dev,
                               float* tile_he_out_dev, float* tile_max_c_out_dev, unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);
/* sx_macenko_augment_masked: sx_macenko_augment's arguments plus the mask: the masked per-tile estimate (own basis: without the
 * concentration bracket pass and the scale stage), then the jitter on masked-in pixels -- the bits of sx_macenko_estimate_masked followed
 * by sx_macenko_apply_masked with the factors.  Masked-out pixels, and tiles without an estimate, are copied by
 * sx_macenko_transform_masked's background rule. */
int sx_macenko_augment_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, const unsigned char* mask_dev,
                              const float* alpha_dev, const float* beta_dev, const float* stain_matrix_dev, const float* target_max_conc_dev,
                              unsigned flags, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- three-stain colour deconvolution with a GIVEN basis (Ruifrok & Johnston: HED, H-DAB, a complemented H&E estimate) ----
 * An extension (HistomicsTK color_deconvolution, scikit-image rgb2hed / hed2rgb): no estimate at all.  The conventions are the Macenko
 * calls': optical density OD_c = -ln((255 x_c + 1) / 240) of the unit value x (uint8: x = u / 255), reconstruction
 * level_c = clamp(240 exp(-OD'_c), 0, 255) cast to the output element by sx_macenko_transform's rules.
 *   basis_dev   n_bases x 9 floats: a basis is (3, 3) row-major as [channel][stain] -- columns are stain vectors, as HE's (3, 2);
 *               n_bases is 1 (one basis for the batch) or n_tiles (row t serves tile t)
 *   C = inverse(basis) OD            three concentrations per pixel; a 3 x 3 basis is invertible, so nothing of OD is dropped
 * Every call is ONE kernel launch on `stream`: nothing else enqueued, no workspace, no host synchronisation, capturable.  Bases, factors
 * and masks are DEVICE memory read by the kernel (a captured graph replayed after new values were written into the same buffers uses
 * the new values).  The inverse is the closed form in fp64 on the device; a SINGULAR basis is NOT detected: its coefficients are Inf /
 * NaN and so are the levels, which the clamp and the casts treat as the Macenko kernels treat them (undefined pixel values, no error).
 * Flags: SX_MACENKO_NORMALIZE_0_1, SX_MACENKO_CHANNELS_LAST, SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16 (uint8 input, one of the two) with
 * their meaning in sx_macenko_apply, SX_MACENKO_CLASSIC (a no-op); any other bit is SX_ERR_BAD_ARG.  All argument errors -- a NULL
 * required pointer, n_bases / n_targets not 1 or n_tiles, one factor pointer without the other, bad flags, SX_MACENKO_CHANNELS_LAST on the
 * masked call -- are SX_ERR_BAD_ARG with a message, before anything is enqueued.
 *
 * sx_deconv_apply:  C' = alpha * C + beta,  OD' = B_out C'  -- one streaming pass, a pixel read, a pixel written.
 *   target_basis_dev     n_targets x 9 floats (n_targets 1 or n_tiles): B_out; NULL: the source basis (n_targets is then ignored)
 *   alpha_dev, beta_dev  n_tiles x 3 floats each, per tile and stain; both or neither (neither: alpha = 1, beta = 0 -- with
 *                        no target the call then rebuilds its input up to rounding) */
int sx_deconv_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                    const float* basis_dev, int64_t n_bases, const float* target_basis_dev, int64_t n_targets,
                    const float* alpha_dev, const float* beta_dev, unsigned flags, void* stream);
/* sx_deconv_apply_masked: the same under an explicit mask (N, H, W), one byte per pixel, non-zero = in (what sx_tissue_mask writes);
 * planar tiles only.  A masked-out pixel is COPIED by sx_macenko_transform_masked's background rule (its input level through the tissue
 * pixels' clamp, cast and / 255: uint8 in, uint8 out is byte-identical there); a tile whose basis row -- or target row, if given --
 * holds a NaN is copied entirely.  Values under masked-out pixels never matter (every use is a select).  The mask is read in packs as
 * wide as the pixel packs where the image pointers, the tile size AND the mask pointer allow it.  All ones: sx_deconv_apply's bits. */
int sx_deconv_apply_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                           const float* basis_dev, int64_t n_bases, const float* target_basis_dev, int64_t n_targets,
                           const float* alpha_dev, const float* beta_dev, const unsigned char* mask_dev, unsigned flags, void* stream);
/* sx_deconv_separate: a pixel is read once; either output may be NULL, not both.
 *   stains_out_dev  (3, N, 3, H, W) of the output element ((3, N, H, W, 3) with SX_MACENKO_CHANNELS_LAST): image i is the tile rebuilt
 *                   from stain i alone, clamp(240 exp(-basis[:, i] C_i)) -- the BITS of sx_deconv_apply with alpha = e_i, beta = 0
 *   conc_out_dev    (N, 3, H, W) float32 ((N, H, W, 3)): C */
int sx_deconv_separate(const void* images_dev, void* stains_out_dev, float* conc_out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                       const float* basis_dev, int64_t n_bases, unsigned flags, void* stream);
/* sx_deconv_combine: sx_deconv_separate's inverse -- a tile rebuilt from (N, 3, H, W) float32 concentrations ((N, H, W, 3) with
 * SX_MACENKO_CHANNELS_LAST, then the output too): out = clamp(240 exp(-basis C), 0, 255) cast to out_dtype (any sx_dtype; uint8
 * truncates as the transform does).  Flags: SX_MACENKO_NORMALIZE_0_1 (fuses / 255; float outputs only -- with uint8 output it is
 * SX_ERR_BAD_ARG), SX_MACENKO_CHANNELS_LAST, SX_MACENKO_CLASSIC (a no-op).  Editing the concentrations in between -- a stain dropped
 * or rescaled -- is what the pair is for. */
int sx_deconv_combine(const float* conc_dev, void* out_dev, int out_dtype, int64_t n_tiles, int64_t height, int64_t width,
                      const float* basis_dev, int64_t n_bases, unsigned flags, void* stream);
/* sx_deconv_quantify: what a deconvolved slide is measured by -- 256-bin INTEGER histograms of the three concentrations, their exact
 * fixed-point sums and the number of counted pixels -- in one streaming pass that reads a pixel once and writes no map.  The
 * concentrations are, bit for bit, the float32 values sx_deconv_separate writes; binning is an exact function of them:
 *   bin_s  = clamp((int)floor(C_s * 2^bin_log2) + zero_bin, 0, 255)   bin b covers [(b - zero_bin) 2^-bin_log2, (b + 1 - zero_bin) 2^-bin_log2);
 *                                                                     bins 0 and 255 also take everything below / above the range
 *   term_s = C_s * 2^16 converted to int32 (round to nearest even, saturating), summed as int64
 *   bin_log2 in [0, 8], zero_bin in [0, 255]  (5 and 64: bins of 1/32 over [-2, 6))
 * A pixel counts iff its three concentrations are finite (a NaN / Inf input element, or 255 x + 1 <= 0, is in no count, no sum and not
 * in `pixels`); a tile whose basis row holds a NaN counts nothing.
 *   out_dev   S x 772 int64, S = n_tiles (per_tile != 0) or 1 (one set pooled over the batch); row s is
 *             [counts: 3 x 256][sums: 3][pixels: 1].  Caller-owned; the call zeroes it in-stream (one hipMemsetAsync) and enqueues ONE
 *             kernel: every word is written.  No workspace.
 * Integers throughout: the result does not depend on the order of the adds -- identical run to run, and rows of different calls add up
 * exactly.  Flags: SX_MACENKO_CHANNELS_LAST (unmasked call only), SX_MACENKO_CLASSIC (a no-op); every other bit is SX_ERR_BAD_ARG
 * (there is no output image). */
int sx_deconv_quantify(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                       const float* basis_dev, int64_t n_bases, int bin_log2, int zero_bin, int per_tile,
                       long long* out_dev, unsigned flags, void* stream);
/* sx_deconv_quantify_masked: the same over the masked-in pixels of an explicit mask (N, H, W), one byte per pixel, non-zero = in; planar
 * tiles only.  Values under masked-out pixels never matter.  The mask is read in packs as wide as the pixel packs where the image pointer,
 * the tile size AND the mask pointer allow it. */
int sx_deconv_quantify_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                              const float* basis_dev, int64_t n_bases, int bin_log2, int zero_bin, int per_tile,
                              long long* out_dev, const unsigned char* mask_dev, unsigned flags, void* stream);
/* sx_deconv_moments: the statistics pass of the stain space -- exact integer first and second moments of the three concentrations, in one
 * streaming pass that reads a pixel once and writes no map (mean / standard deviation matching of concentrations, statistics-space
 * augmentation).  The concentrations are, bit for bit, the float32 values sx_deconv_separate writes and sx_deconv_quantify bins, and
 * a pixel counts under sx_deconv_quantify's rule: three finite concentrations (and, masked, its mask byte set); a tile whose basis row
 * holds a NaN counts nothing.  Per counted pixel and stain:
 *   t_s = C_s * 2^16 converted to int32 (round to nearest even, saturating) -- sx_deconv_quantify's term;   sums_s    += t_s
 *   u_s = clamp(t_s, -2^22, 2^22);                                                                          squares_s += (u_s * u_s) >> 8
 * so `sums` has the unit 2^-16 and `squares` the unit 2^-24 (floored; a concentration beyond +-64 enters the squares as 64).
 *   out_dev   S x 7 int64, S = n_tiles (per_tile != 0) or 1 (one set pooled over the batch); row s is [sums: 3][squares: 3][pixels: 1].
 *             Caller-owned; the call zeroes it in-stream (one hipMemsetAsync) and enqueues ONE kernel: every word is written.  No workspace.
 *             On a stream that is being captured the zeroes come from a small clearing launch instead of the memset: with HIP 7.0 /
 *             ROCm 7.2 a memset node's replay depends on what was launched since the previous replay (tools/probe_graph_memset.py,
 *             profiles/graph_memset_probe.txt: a graph of one hipMemsetAsync writes wrong bytes on every replay that follows a
 *             reduction and its read-back), a kernel node replays its own arguments.
 * Integers throughout: the result does not depend on the order of the adds -- identical run to run, and rows add up exactly over tiles,
 * batches, slides and ranks.  No overflow below 2^27 counted pixels per row even if every term is clamped (2^63 / 2^36; the sums: 2^63 /
 * 2^31 pixels).  The floor biases a pixel's C^2 by less than 2^-24, downwards.
 * Arguments, layouts (SX_MACENKO_CHANNELS_LAST: unmasked call only), the five element types, per-tile bases (n_bases = 1 or n_tiles) and
 * flags (SX_MACENKO_CHANNELS_LAST, SX_MACENKO_CLASSIC as a no-op; every other bit is SX_ERR_BAD_ARG) are sx_deconv_quantify's. */
int sx_deconv_moments(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                      const float* basis_dev, int64_t n_bases, int per_tile, long long* out_dev, unsigned flags, void* stream);
/* sx_deconv_moments_masked: the same over the masked-in pixels of an explicit mask (N, H, W), one byte per pixel, non-zero = in; planar
 * tiles only.  Values under masked-out pixels never matter. */
int sx_deconv_moments_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                             const float* basis_dev, int64_t n_bases, int per_tile, long long* out_dev,
                             const unsigned char* mask_dev, unsigned flags, void* stream);

/* ---- HSV colour jitter: per-tile hue, saturation and value (Tellez et al.'s HSV-light / HSV-strong; RandStainNA's third space) ----
 * An extension: no statistics and no estimate, one row of five floats per tile.  All arithmetic is float32 on 0-255 levels; r, g, b are
 * the input levels (uint8: the byte; floats: 255 x) clamped to [0, 255]:
 *   M = max, m = min, C = M - m;   s = C / M (0 where M <= 0)
 *   h6 in [0, 6): 0 where C == 0; (g - b) / C, plus 6 if negative, where M == r; 2 + (b - r) / C where M == g; 4 + (r - g) / C otherwise
 *   h6' = h6 + 6 dh, reduced into [0, 6) by x - 6 floor(x / 6);   s' = clamp(a_s s + b_s, 0, 1);   V' = 255 clamp(a_v M / 255 + b_v, 0, 1)
 *   for n = 5, 3, 1 (r, g, b):  k = h6' + n, minus 6 where k >= 6;  t = clamp(min(k, 4 - k), 0, 1);  out = V' - V' s' t
 *   rows_dev   n_rows x 5 floats (dh, a_s, b_s, a_v, b_v), dh in turns; n_rows is 1 (one row for the batch) or n_tiles (row t serves
 *              tile t).  (0, 1, 0, 1, 0) is the identity.
 * Output: a float element gets the level by sx_macenko_transform's rules (SX_MACENKO_NORMALIZE_0_1 fuses / 255).  An 8-bit level -- uint8
 * output, and the level a uint8 tile's result is quantised to before SX_MACENKO_OUT_BF16 / _OUT_F16 / the / 255 -- is ROUNDED TO NEAREST,
 * unlike the stain calls, which truncate: with rounding the identity row returns every one of the 2^24 uint8 colours exactly (the
 * float32 round trip is off by up to 1.8e-4 of a level, which truncation turns into a level).
 * Copies: a pixel with a NaN in any channel, and every pixel of a tile whose row has a non-finite member (NaN, Inf: "leave this tile"),
 * are copied by sx_macenko_transform_masked's background rule -- the input level through the clamp, the cast and / 255 (uint8 in, uint8
 * out is byte-identical there).
 * Each call is ONE kernel launch on `stream`: nothing else enqueued, no workspace, no host synchronisation, capturable.  Rows and masks
 * are DEVICE memory read by the kernel (a captured graph replayed after new values were written into the same buffers uses the new
 * values).  Flags: SX_MACENKO_NORMALIZE_0_1, SX_MACENKO_CHANNELS_LAST, SX_MACENKO_OUT_BF16 / SX_MACENKO_OUT_F16 (uint8 input, one of the
 * two) with their meaning in sx_deconv_apply, SX_MACENKO_CLASSIC (a no-op); any other bit is SX_ERR_BAD_ARG.  All argument errors -- a
 * NULL pointer, a non-positive size, n_rows not 1 or n_tiles, bad flags, SX_MACENKO_CHANNELS_LAST on the masked call -- are
 * SX_ERR_BAD_ARG with a message, an unknown dtype is SX_ERR_DTYPE, before anything is enqueued. */
int sx_hsv_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                 const float* rows_dev, int64_t n_rows, unsigned flags, void* stream);
/* sx_hsv_apply_masked: the same under an explicit mask (N, H, W), one byte per pixel, non-zero = in (what sx_tissue_mask writes); planar
 * tiles only.  A masked-out pixel is copied by the background rule; values under masked-out pixels never matter (every use is a select).
 * The mask is read in packs as wide as the pixel packs where the image pointers, the tile size AND the mask pointer allow it.  All ones:
 * sx_hsv_apply's bits. */
int sx_hsv_apply_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                        const float* rows_dev, int64_t n_rows, const unsigned char* mask_dev, unsigned flags, void* stream);

/* ---- Tone jitter: per-tile brightness, contrast, gamma and additive Gaussian noise (the "BC" member and the noise of Tellez et al.'s set) ----
 * An extension: one row of four floats per tile, and one 64-bit seed per tile where noise is asked for.
 *   rows_dev   n_rows x 4 floats (a, b, gamma, sigma); n_rows is 1 (one row for the batch) or n_tiles (row t serves tile t).
 *              (1, 0, 1, 0) is the identity.
 *   seeds_dev  NULL: no noise (a kernel without the generator), or n_tiles int64 in device memory.  A tile with sigma == 0 adds nothing.
 * All arithmetic is float32 on 0-255 levels, every fused multiply-add written out; x is the input level (uint8: the byte; floats: 255 x)
 * clamped to [0, 255].  For each channel of each pixel:
 *   1. t = clamp(fma(a, x, 255 b), 0, 255): a = 1, b = 0 gives x exactly.  (255 b is carried as the float32 pair fl(255 b) and its exact
 *      remainder, the remainder added after the fused sum: t is within two roundings of a x + 255 b even where the two cancel.)
 *   2. where gamma != 1: t = 255 (t / 255)^gamma, 0 staying 0 -- 255 exp2f(gamma log2f(t / 255)); gamma == 1 is a select, not an evaluation.
 *   3. where noise is on: t = clamp(t + 255 sigma z, 0, 255).
 * The noise.  For pixel p = y W + x of a tile with seed s:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (p & 0xffffffff, p >> 32, 0, 0), key = (s & 0xffffffff, (s >> 32) & 0xffffffff))
 *   u(w) = (2 (w >> 9) + 1) 2^-24, exact in float32 and strictly inside (0, 1)
 *   rho = sqrt(-2 ln u(w0)),  z_r = rho cos(2 pi u(w1)),  z_g = rho sin(2 pi u(w1));  from (w2, w3) the same way z_b (cosine), z_s (sine)
 *   shared_noise == 0: channels r, g, b get z_r, z_g, z_b;  shared_noise != 0: all three channels get z_s.
 * One Philox call per pixel serves both modes.  The field depends on (seed, p) only: not on the layout, the pack width, the mask, the
 * launch geometry or the tile's place in the batch.
 * Output: sx_hsv_apply's rule -- an 8-bit level is ROUNDED TO NEAREST, so the identity row returns every byte; SX_MACENKO_NORMALIZE_0_1,
 * SX_MACENKO_OUT_BF16 / _OUT_F16 (uint8 input) and SX_MACENKO_CHANNELS_LAST (unmasked only) as there.
 * Copies, by sx_hsv_apply's background rule and with its bits: a pixel with a NaN in any channel; a masked-out pixel; every pixel of a
 * tile whose row has a non-finite member, gamma <= 0 or sigma < 0 ("leave this tile"), whatever its seed.  Every use of a value that may be
 * NaN is a select.
 * Each call is ONE kernel launch on `stream`: no workspace, no atomics, no memset, capturable.  Rows, seeds and masks are DEVICE memory
 * read by the kernel: a replayed graph uses whatever was written to them.  Flags, flag checks and argument errors are sx_hsv_apply's. */
int sx_tone_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                  const float* rows_dev, int64_t n_rows, const long long* seeds_dev, int shared_noise, unsigned flags, void* stream);
/* sx_tone_apply_masked: the same under an explicit mask (N, H, W), one byte per pixel, non-zero = in; planar tiles only.  A masked-out
 * pixel is copied; a masked-in pixel has sx_tone_apply's bits (the noise of a pixel does not depend on the mask). */
int sx_tone_apply_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                         const float* rows_dev, int64_t n_rows, const long long* seeds_dev, int shared_noise,
                         const unsigned char* mask_dev, unsigned flags, void* stream);

/* ---- Grey statistics: pixels, sum Y, sum Y^2 per tile or per batch (brightness and RMS contrast; the pivot of a contrast change) ----
 * statistics_out_dev: S x 3 int64 [pixels, sum Y, sum Y^2], S = n_tiles, or 1 with pooled != 0.  Y is sx_grey_map's level (a pixel with a
 * NaN channel has Y = 0 and is counted).  Every pixel is counted; in the masked form only the pixels whose mask byte is non-zero (planar
 * tiles only there: channels_last must be 0).  ONE streaming launch reads the tile once and writes no map: 32-bit lane sums over chunks
 * that cannot overflow, a wave reduction, one 64-bit integer add per word and workgroup into words cleared first -- by a memset, or by a
 * small clearing launch while the stream is being captured (sx_deconv_moments's rule).  Integers only: the result is independent of the
 * order and poolable by addition.  Argument errors (a NULL pointer, a non-positive size, too many tiles) are SX_ERR_BAD_ARG, an unknown
 * dtype SX_ERR_DTYPE, before anything is enqueued. */
int sx_grey_statistics(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last, int pooled,
                       long long* statistics_out_dev, void* stream);
int sx_grey_statistics_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last, int pooled,
                              const unsigned char* mask_dev, long long* statistics_out_dev, void* stream);

/* ---- Gaussian blur with a sigma per tile (the blur of Tellez et al.'s augmentation set; the other half of the focus measurement) ----
 * An extension: the reference has none.  One float32 sigma per tile; each channel plane is filtered on its own, a pixel never sees
 * another tile.
 *   sigmas_dev n_rows floats; n_rows is 1 (one sigma for the batch) or n_tiles (sigma t serves tile t).
 *   Radius     R = min((int)(4 sigma + 0.5), 16) of the float32 sigma, the sum taken exactly (scipy.ndimage.gaussian_filter, truncate = 4.0:
 *              R = 0 for every sigma below 0.125).  SX_BLUR_MAX_SIGMA = 4:
 *              a larger finite sigma is clamped to 4 (the rows are device memory: nothing is refused).
 *   Taps       w_i = exp(-i^2 / (2 sigma^2)), i = -R..R, divided by their sum, in float32: all positive, a convex combination.
 *   Borders    reflected without repeating the edge inside the pixel's own tile, folded as often as needed (period 2 (n - 1); an axis of
 *              length 1 maps to 0): scipy's mode="mirror", torch's "reflect" padding.
 *   Arithmetic separable, rows then columns, float32, on the values as the element type stores them: a uint8 byte is its level, a float
 *              element is taken as it is (no x 255: the filter is linear).  Per pass acc = w_0 x_0, then acc = fma(w_i, x_-i + x_+i, acc).
 * Output: the result through sx_macenko_transform's output rule (the cast; SX_MACENKO_NORMALIZE_0_1 fuses / 255; uint8 input may ask for
 * SX_MACENKO_OUT_BF16 / _OUT_F16).  An 8-bit level is ROUNDED TO NEAREST, as in sx_hsv_apply: a blur that changes nothing returns the tile.
 * Copies: a tile whose sigma is NaN, infinite or <= 0, or whose R is 0 (sigma < 0.125), is copied -- the stored element through the output
 * rule, no clamp; where the output element is the input element and nothing is divided, the element's bits (NaN payloads, -0.0).
 * Non-finite pixels are not special: a NaN pixel spreads over its (2 R + 1)^2 window as IEEE arithmetic takes it, and over nothing else.
 * Each call is ONE kernel launch on `stream`: nothing else enqueued, no workspace, no host synchronisation, capturable; neither pass goes
 * through device memory.  Sigmas and masks are DEVICE memory read by the kernel.  Flags and argument errors as sx_hsv_apply. */
#define SX_BLUR_MAX_SIGMA 4.0f
int sx_gaussian_blur(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                     const float* sigmas_dev, int64_t n_rows, unsigned flags, void* stream);
/* sx_gaussian_blur_masked: the same under an explicit mask (N, H, W), one byte per pixel, non-zero = in; planar tiles only.  The mask
 * selects which OUTPUT pixels are written from the blur -- a masked-out pixel is copied --; the taps read every pixel and the weights are
 * not renormalised.  All ones: sx_gaussian_blur's bits. */
int sx_gaussian_blur_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                            const float* sigmas_dev, int64_t n_rows, const unsigned char* mask_dev, unsigned flags, void* stream);

/* ---- JPEG compression round trip with a quality per tile (the compression artefacts every whole-slide pipeline meets: 8 x 8 blocks,
 * smeared chroma) ----
 * An extension: the reference has none.  The output is, BIT FOR BIT, what baseline JPEG as libjpeg implements it -- Pillow's
 * Image.save(..., "JPEG", quality=q, subsampling=s) followed by Image.open -- decodes to.  The lossy part of that codec is 32-bit integer
 * arithmetic and its entropy coder is lossless, so encode and decode are fused and no bitstream is produced.  A pixel never sees another tile.
 * All arithmetic is int32, >> is arithmetic, D(x, n) = (x + (1 << (n - 1))) >> n.
 *   qualities_dev n_rows floats; n_rows is 1 (one quality for the batch) or n_tiles.  q = min((int)quality, 100).  A quality that is NaN,
 *              infinite or < 1 leaves its tile (see Copies).  Quality 100 is NOT the identity: its tables are all ones, the colour
 *              conversion and the two transforms still round.
 *   subsampling 0: 4:4:4, 2: 4:2:0 (Pillow's numbering), one value per call.
 *   Input      a uint8 byte is its level; a float element x, converted to float32, is clamp(rint(255 x), 0, 255); a NaN is level 0
 *              (sx_grey_statistics' rule).  A codec sees 8-bit levels: this quantisation is part of the feature.
 *   Colour     (JFIF, libjpeg's 16-bit tables)  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *              Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16,  Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16.
 *   Planes     a plane that is not subsampled is extended to multiples of 8 by replicating its last column and row.  4:2:0, each chroma
 *              plane, in this order: (1) the last column replicated up to a multiple of 16 columns; (2) the last row replicated to an even
 *              height; (3) the 2 x 2 mean (a + b + c + d + bias) >> 2, bias 1 in even output columns and 2 in odd ones; (4) the last
 *              DOWNSAMPLED row replicated down to a multiple of 8 rows.
 *   Tables     scale = 5000 / q (integer division) for q < 50, else 200 - 2 q;  Q[i] = clamp((base[i] * scale + 50) / 100, 1, 255); base
 *              is Annex K's luminance table for Y, its chrominance table for Cb and Cr, in row-major order:
 *                luminance    16 11 10 16 24 40 51 61 / 12 12 14 19 26 58 60 55 / 14 13 16 24 40 57 69 56 / 14 17 22 29 51 87 80 62 /
 *                             18 22 37 56 68 109 103 77 / 24 35 55 64 81 104 113 92 / 49 64 78 87 103 121 120 101 / 72 92 95 98 112 100 103 99
 *                chrominance  17 18 24 47 99 99 99 99 / 18 21 26 66 99 99 99 99 / 24 26 56 99 99 99 99 99 / 47 66 99 99 99 99 99 99 / then 99
 *   Forward    libjpeg's jfdctint on level - 128 per 8 x 8 block, rows then columns (CONST_BITS 13, PASS1_BITS 2).  With t0..t3 the sums
 *              d0+d7, d1+d6, d2+d5, d3+d4 and t7..t4 the differences d0-d7 .. d3-d4:  t10 = t0+t3, t13 = t0-t3, t11 = t1+t2, t12 = t1-t2;
 *              outputs 0 and 4 are (t10 +- t11) * 4 in the row pass, D(t10 +- t11, 2) in the column pass;  z1 = (t12+t13) * 4433, output 2
 *              is D(z1 + t13 * 6270, n), output 6 D(z1 - t12 * 15137, n), n = 11 (rows) / 15 (columns).  Odd part:  z1 = t4+t7, z2 = t5+t6,
 *              z3 = t4+t6, z4 = t5+t7, z5 = (z3+z4) * 9633;  t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;  z1 *= -7373, z2 *= -20995,
 *              z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;  outputs 7, 5, 3, 1 are D(t4+z1+z3, n), D(t5+z2+z4, n), D(t6+z2+z3, n),
 *              D(t7+z1+z4, n).  The result carries a factor of 8.
 *   Quantise   k = sign(c) ((|c| + (8 Q >> 1)) / (8 Q)), integer division; dequantise k Q.
 *   Inverse    jidctint, columns then rows, the same even / odd structure on the dequantised values: the even part starts from
 *              (in0 +- in4) * 8192, the z of inputs 2 and 6 as above, the odd inputs taken in the order 7, 5, 3, 1 through the same twelve
 *              constants; the column pass descales by D(., 11), the row pass by D(., 18); then clamp(. + 128, 0, 255).
 *   Chroma up  (4:2:0) libjpeg's "fancy" triangle filter on the decoded chroma plane cropped to ceil(H/2) x ceil(W/2), edges replicated:
 *              for the upper / lower output row of a pair t = 3 * row + (row above / row below); the even output column is
 *              (3 t + t_left + 8) >> 4, the odd one (3 t + t_right + 7) >> 4 (first column (4 t + 8) >> 4, last (4 t + 7) >> 4).
 *              NARROW TILES: where the cropped chroma plane is at most 2 columns wide (W <= 4) libjpeg does not filter: every chroma
 *              sample is replicated 2 x 2 (checked against Pillow for every H in 1..19, W in 1..4).
 *   RGB        with cb, cr minus 128:  R = Y + ((91881 cr + 32768) >> 16),  B = Y + ((116130 cb + 32768) >> 16),
 *              G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), each clamped to 0..255.
 * Output: the 8-bit level through sx_hsv_apply's output rule (the cast; SX_MACENKO_NORMALIZE_0_1 fuses / 255; uint8 input may ask for
 * SX_MACENKO_OUT_BF16 / _OUT_F16); the level is an integer, nothing is rounded.
 * Copies: a tile whose quality is NaN, infinite or < 1 is copied by sx_hsv_apply's copy rule -- the input level, clamped to [0, 255],
 * through the output rule; uint8 in, uint8 out: the same bytes.
 * Each call is ONE kernel launch on `stream`: nothing else enqueued, no bitstream, no workspace, no host synchronisation, capturable;
 * nothing goes through device memory between the colour conversion and the final store.  Qualities and masks are DEVICE memory read by the
 * kernel.  Flags as sx_gaussian_blur.  Argument errors, in this order and before anything is enqueued: null pointers, non-positive sizes,
 * the 2^32 limit, n_rows, subsampling not 0 or 2 (SX_ERR_BAD_ARG), flags, the layout flag on the masked call, then the dtype. */
int sx_jpeg_roundtrip(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                      const float* qualities_dev, int64_t n_rows, int subsampling, unsigned flags, void* stream);
/* sx_jpeg_roundtrip_masked: the same under an explicit mask (N, H, W), one byte per pixel, non-zero = in; planar tiles only.  A masked-out
 * pixel is copied by the copy rule above; the codec reads every pixel.  All ones: sx_jpeg_roundtrip's bits. */
int sx_jpeg_roundtrip_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                             const float* qualities_dev, int64_t n_rows, int subsampling, const unsigned char* mask_dev, unsigned flags, void* stream);

/* ---- Affine warp with a row per tile (the geometric half of Tellez et al.'s augmentation set: quarter turns, flips, rotation, scale,
 * shear, translation; crop, pad and resize in the same launch) ----
 * An extension: the reference has none.  The source tile is height x width, the output tile out_height x out_width.
 *   rows_dev   n_rows x 6 floats (a, b, c, d, e, f); n_rows is 1 (one row for the batch) or n_tiles (row t serves tile t).  The row maps
 *              an OUTPUT pixel to the SOURCE position, pixel centres at integers (scipy.ndimage.affine_transform, cv2.warpAffine with
 *              WARP_INVERSE_MAP, grid_sample(align_corners=True) un-normalised): for output column x and row y, in float32,
 *              sx = fmaf(a, x, fmaf(b, y, c)),  sy = fmaf(d, x, fmaf(e, y, f)).
 *   Anchor     a row with a NaN or an infinity means "leave this tile": it is replaced by (1, 0, (W - OW) div 2, 0, 1, (H - OH) div 2),
 *              floor division -- a copy where the sizes are equal, else the centre crop, or the centre pad by the border rule.
 *   Limit      a coordinate that is not finite or exceeds SX_WARP_MAX_COORD = 2^22 in magnitude makes the pixel `fill`, in both border
 *              modes (tested in float32 before any integer is formed).  No value of a row makes the kernel read outside the tile.
 *   Borders    SX_WARP_MIRROR: reflected without repeating the edge inside the tile, folded as often as needed (period 2 (n - 1), an
 *              axis of length 1 maps to 0): scipy's "mirror", torch's "reflection" with align_corners=True.  SX_WARP_CONSTANT: a tap
 *              outside the tile is `fill` (scipy's "grid-constant", cv2's BORDER_CONSTANT).  `fill`: a finite float32 on the element's
 *              own scale -- a level for uint8 tiles (clamped to 0..255), taken as it is for float tiles --, through the output rule.
 *   Bilinear   x0 = floorf(sx), fx = sx - x0, y0 and fy likewise; the four taps through the border rule, as the element type stores
 *              them (a uint8 byte is its level, a float element as it is; no x 255):
 *              top = fmaf(fx, v01 - v00, v00), bot = fmaf(fx, v11 - v10, v10), v = fmaf(fy, bot - top, top).  fx == 0 and fy == 0:
 *              the stored element, copied.  Non-finite pixels are not special.
 *   Nearest    xi = floorf(sx + 0.5f), yi likewise (scipy's order=0): the stored element at (xi, yi) through the border rule, copied.
 * Output: sx_gaussian_blur's rule (an 8-bit level ROUNDED TO NEAREST; SX_MACENKO_NORMALIZE_0_1; SX_MACENKO_OUT_BF16 / _OUT_F16 for
 * uint8 input); a copied element keeps its bits where the output element is the input element and nothing is divided (NaN payloads,
 * -0.0).  out_dev MUST NOT overlap images_dev.
 * Each call is ONE kernel launch on `stream`: nothing else enqueued, no workspace, no host synchronisation, capturable.  Rows are DEVICE
 * memory read by the kernel.  Flags as sx_gaussian_blur.  Argument errors, in this order and before anything is enqueued: null pointers,
 * sizes not positive, N*H*W or N*OH*OW at or above 2^32, n_rows, interpolation / border, fill, flags, dtype. */
#define SX_WARP_NEAREST 0
#define SX_WARP_BILINEAR 1
#define SX_WARP_MIRROR 0
#define SX_WARP_CONSTANT 1
#define SX_WARP_MAX_COORD 4194304.0f
int sx_affine_warp(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                   int64_t out_height, int64_t out_width, const float* rows_dev, int64_t n_rows,
                   int interpolation, int border, float fill, unsigned flags, void* stream);
/* sx_affine_warp_mask: a mask (N, H, W), one byte per pixel, warped WITH its tile -- it does not select pixels --: nearest, bytes moved
 * as bytes (labels 0..255 survive), SX_WARP_MIRROR or SX_WARP_CONSTANT with the byte `fill` (0..255).  The nearest sx_affine_warp of
 * the same plane and rows gives the same bytes: an image and its mask warped by the same rows stay aligned. */
int sx_affine_warp_mask(const unsigned char* mask_dev, unsigned char* out_dev, int64_t n_tiles, int64_t height, int64_t width,
                        int64_t out_height, int64_t out_width, const float* rows_dev, int64_t n_rows,
                        int border, int fill, void* stream);

/* ---- Elastic deformation with a control grid per tile (the other half of Tellez et al.'s "morphology" set), fused with the affine
 * warp: scale, rotation, elastic deformation and the crop are ONE launch ----
 * An extension: the reference has none.  Everything of sx_affine_warp holds; the coordinate alone gains a displacement.
 *   grids_dev  n_grids x 2 x GH x GW floats, n_grids 1 (one grid for the batch) or n_tiles: plane 0 holds dx, plane 1 dy, in SOURCE
 *              pixels.  GH = (out_height - 1) div cell + 4, GW = (out_width - 1) div cell + 4; control column j sits at output column
 *              (j - 1) * cell, rows likewise.
 *   cell       the control spacing in OUTPUT pixels, SX_ELASTIC_MIN_CELL (4) .. SX_ELASTIC_MAX_CELL (4096), one for the batch.
 *   Displacement  for output pixel (x, y): jx = x div cell, tx = float(x - jx * cell) / float(cell), jy and ty likewise; with the
 *              uniform cubic B-spline weights B0 = (1 - t)^3 / 6, B1 = (3 t^3 - 6 t^2 + 4) / 6, B2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6,
 *              B3 = t^3 / 6:  dx = sum_l B_l(ty) * (sum_k B_k(tx) * P0[jy + l][jx + k]), dy from plane 1 -- float32, the x pass first,
 *              every operation as stainx_amd/csrc/elastic.hpp writes it out.
 *   Coordinates   sx = fmaf(a, x, fmaf(b, y, c)) + dx,  sy = fmaf(d, x, fmaf(e, y, f)) + dy; then sx_affine_warp's rule: a coordinate
 *              that is not finite or beyond SX_WARP_MAX_COORD (a NaN, an infinite or a huge displacement) gives `fill`.
 *   A row with a NaN or an infinity leaves its tile as in sx_affine_warp (copy, centre crop, centre pad); its grid is not read.
 *   A grid of zeros gives sx_affine_warp's output bit for bit.  No grid and no row makes the kernel read outside the tile or the grid.
 * ONE kernel launch on `stream`, nothing else enqueued, no workspace, capturable; rows and grids are DEVICE memory read by the kernel.
 * Argument errors as sx_affine_warp's, with a null grids_dev, n_grids and cell after interpolation / border and before fill. */
#define SX_ELASTIC_MIN_CELL 4
#define SX_ELASTIC_MAX_CELL 4096
int sx_elastic_warp(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                    int64_t out_height, int64_t out_width, const float* rows_dev, int64_t n_rows,
                    const float* grids_dev, int64_t n_grids, int cell,
                    int interpolation, int border, float fill, unsigned flags, void* stream);
/* sx_elastic_warp_mask: the mask (N, H, W) warped WITH its tile, as sx_affine_warp_mask: nearest, bytes moved as bytes, the same
 * coordinates as the nearest sx_elastic_warp of the same rows and grids. */
int sx_elastic_warp_mask(const unsigned char* mask_dev, unsigned char* out_dev, int64_t n_tiles, int64_t height, int64_t width,
                         int64_t out_height, int64_t out_width, const float* rows_dev, int64_t n_rows,
                         const float* grids_dev, int64_t n_grids, int cell,
                         int border, int fill, void* stream);

/* Per-tile intermediates of the LAST sx_macenko_transform / sx_macenko_augment / sx_macenko_separate / sx_macenko_fit that used `workspace_dev`
 * (tests compare them with the oracle).  params_out_dev: n_groups x SX_MACENKO_PARAM_FLOATS floats:
 *   [0] n_selected  [1] used_all_pixels  [2..7] plane vectors (3,2)  [8] phi_lo  [9] phi_hi
 *   [10..15] HE_source (3,2)  [16..17] maxC  [18] select paths taken (bit i: slot i fell back to the
 *   full-tile radix select)  [19..22] candidates gathered per slot  [23..31] covariance (3,3)
 *   [32..47] diagnostic stage timestamps of the per-tile kernels, microseconds                     */
#define SX_MACENKO_PARAM_FLOATS 48
int sx_macenko_tile_params(const void* workspace_dev, int64_t n_groups, float* params_out_dev, void* stream);

/* Pooled fit over a batch that is SHARDED ACROSS RANKS (one process per GPU).  The host all-reduces
 * (SUM) the small buffers between the calls; every rank ends with identical (HE, maxC):
 *   sx_macenko_dfit_moments   local 20 fp64 raw moments            -> all-reduce
 *   sx_macenko_dfit_begin     plane vectors from the global moments, starts the angle selection
 *   repeat 4x: sx_macenko_dfit_histogram(stage)  local 2 x 256 u64 bins of the current radix round
 *              -> all-reduce -> sx_macenko_dfit_advance(stage)     (stage 0: phi@1,phi@99; stage 1: C0@99,C1@99)
 *   sx_macenko_dfit_result    copies HE (6 floats) and maxC (2 floats) out of the state             */
size_t sx_macenko_dfit_state_bytes(void);
int sx_macenko_dfit_moments(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                            double* moments_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_macenko_dfit_begin(const double* moments_dev, void* state_dev, void* stream);
int sx_macenko_dfit_histogram(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                              const void* state_dev, int stage, unsigned long long* hist_out_dev, void* stream);
int sx_macenko_dfit_advance(void* state_dev, int stage, const unsigned long long* hist_dev, void* stream);
int sx_macenko_dfit_result(const void* state_dev, float* he_out_dev, float* max_c_out_dev, void* stream);

/* The same pooled fit across ranks on the BRACKET machinery of sx_macenko_fit: three passes over the local tiles
 * instead of nine.  Every rank calls the steps in lockstep; the host moves four small device buffers in between
 * (`stainx_amd/distributed.py` does it with torch.distributed):
 *   sx_macenko_pfit_stats    local moments (10 doubles) -> all-reduce(SUM); local sample (3 x 4096 floats, the first
 *                            sx_macenko_pfit_sample_count() columns valid) -> all-gather; every rank builds the same
 *                            4096-column union (every world-th column of every rank)
 *   sx_macenko_pfit_plane    global moments + n_all (pixels over all ranks) + union sample -> plane, angle brackets
 *   sx_macenko_pfit_pass     stage 0 angle / 1 concentration: local counts and histogram (SX_PFIT_SUMS int64 values)
 *                            -> all-reduce(SUM)
 *   sx_macenko_pfit_gather   global sums in; local candidates of the picked bin out (2 x share keys, 2 counts; share =
 *                            SX_PFIT_COMPACT / world) -> all-gather
 *   sx_macenko_pfit_finish   gathered candidates [world][2][share], counts [world][2] -> exact percentiles;
 *                            stage 0: stain vectors and concentration brackets, stage 1: HE, maxC and *status_out
 *                            (non-zero: a bracket did not hold somewhere -- repeat with the sx_macenko_dfit_* rounds)
 * Integer counts and an order-independent selection: every rank ends with the same bits. */
#define SX_PFIT_SUMS 1033
#define SX_PFIT_COMPACT 32768
int sx_macenko_pfit_sample_count(int64_t n_tiles, int64_t height, int64_t width);
int sx_macenko_pfit_stats(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                          double* moments_out_dev, float* sample_out_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
int sx_macenko_pfit_plane(const double* moments_dev, long long n_all, const float* sample_union_dev, int sample_count,
                          int64_t n_tiles, int64_t height, int64_t width, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
int sx_macenko_pfit_pass(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int stage,
                         long long n_all, int sample_count, long long* sums_out_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream);
int sx_macenko_pfit_gather(const long long* sums_global_dev, int stage, long long n_all, int sample_count,
                           int64_t n_tiles, int64_t height, int64_t width, int share, unsigned* compact_out_dev,
                           int* counts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_macenko_pfit_finish(const unsigned* gathered_compact_dev, const int* gathered_counts_dev, int world, int share, int stage,
                           long long n_all, int sample_count, int64_t n_tiles, int64_t height, int64_t width,
                           float* he_out_dev, float* max_c_out_dev, int* status_out_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);

/* The same steps with what travels through a collective PACKED AND UNPACKED BY THE LIBRARY: one contiguous record per rank and
 * exchange, so the host side is an all-gather / all-reduce of a buffer it never looks into (the unpacked steps above cost the
 * host a dozen small tensor operations per exchange: a third of a pooled fit_transform step).
 *   stats record  [int64 tiles | 10 fp64 moments | 3 x 4096 fp32 sample]                  SX_PFIT_STATS_RECORD_BYTES, 8-byte aligned
 *   stage record  [int32 count, count, stale flag | 2 x share uint32 candidate keys]      (3 + 2 share) x 4 bytes
 *   sx_macenko_pfit_stats_packed   the rank's stats record -> all-gather
 *   sx_macenko_pfit_plane_packed   every rank's record [world][record]: moments added up in rank order, the union sample (every
 *                                  world-th column of every rank, ranks one after the other, cut at 4096; sample_counts_host[r] =
 *                                  sx_macenko_pfit_sample_count of rank r's tiles, a HOST array), and -- if expected_tiles_dev
 *                                  is given -- *stale_out_dev = 1 when some rank's tile count differs from it (the host may take
 *                                  the counts of the last call on trust and have them checked here), else 0
 *   sx_macenko_pfit_gather_packed  as sx_macenko_pfit_gather; writes the rank's stage record, stale_flag_dev (may be null) into it
 *   sx_macenko_pfit_finish_packed  as sx_macenko_pfit_finish on the gathered stage records [world][3 + 2 share]; any rank's stale
 *                                  flag sets bit 4 (16) of *status_out (bits 0-3: brackets that did not hold) */
#define SX_PFIT_STATS_RECORD_BYTES 49240
int sx_macenko_pfit_stats_packed(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                                 void* record_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_macenko_pfit_plane_packed(const void* gathered_records_dev, int world, const int* sample_counts_host,
                                 const long long* expected_tiles_dev, int* stale_out_dev, long long n_all, int sample_count,
                                 int64_t n_tiles, int64_t height, int64_t width, void* workspace_dev, size_t workspace_bytes,
                                 void* stream);
int sx_macenko_pfit_gather_packed(const long long* sums_global_dev, int stage, long long n_all, int sample_count,
                                  int64_t n_tiles, int64_t height, int64_t width, int share, const int* stale_flag_dev,
                                  unsigned* record_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_macenko_pfit_finish_packed(const unsigned* gathered_records_dev, int world, int share, int stage, long long n_all,
                                  int sample_count, int64_t n_tiles, int64_t height, int64_t width, float* he_out_dev,
                                  float* max_c_out_dev, int* status_out_dev, void* workspace_dev, size_t workspace_bytes,
                                  void* stream);

/* ---------------------------------------------------------------- Reinhard -----------------------
 * Replaces stainx_cuda_torch.reinhard (bindings.cpp:32) with the numerics of ReinhardTorch
 * (torch_backend.py:304-355): LAB statistics pooled over the whole batch, unbiased std. */
size_t sx_reinhard_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
/* ... with room for the 8-bit codes of a float32 batch (+ 3 bytes per pixel): sx_reinhard_transform(_ready) then leaves the tiles that
 * consist of grey levels (float(k) / 255 in every element) as bytes in its first pass and reads those in its second -- same bits, a
 * quarter of the second pass's input.  Every entry point also accepts the smaller workspace above and then runs without. */
size_t sx_reinhard_workspace_bytes_for(int dtype, int64_t n_tiles, int64_t height, int64_t width);
int sx_reinhard_fit(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                    float* mean_out_dev, float* std_out_dev, void* workspace_dev, size_t workspace_bytes,
                    void* stream);
int sx_reinhard_transform(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                          int64_t width, const float* ref_mean_dev, const float* ref_std_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* The transform for a workspace in the READY state: zero-filled once by sx_reinhard_workspace_init() (or by the caller), and since then
 * only touched by completed calls of this section -- each leaves it ready again.  It skips the launch that clears the arrival
 * counters in front of the statistics pass (~4 us of a 130 us call on 64 x 3 x 512 x 512 float32).  The plain calls above accept ANY
 * workspace contents and leave it ready as well.  A ready call on a workspace that was not ready is noticed on the device (the apply
 * pass does not find the statistics of its own statistics pass): bit 0 of the uint32 at byte sx_reinhard_workspace_status_offset()
 * is set; the output of such a call is not to be used.  The state a ready call relies on (the arrival counters) lies at a place that does
 * NOT depend on the batch's shape (batches of up to 4096 tiles; a larger batch is served as by the plain call), so calls of different
 * shapes may alternate on one ready workspace -- also when replayed from a captured graph.  No reference counterpart (the reference
 * keeps no state between calls). */
int sx_reinhard_workspace_init(void* workspace_dev, size_t workspace_bytes, void* stream);
size_t sx_reinhard_workspace_status_offset(void);
int sx_reinhard_transform_ready(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                                int64_t width, const float* ref_mean_dev, const float* ref_std_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream);

/* Batch statistics pooled across ranks: sx_reinhard_sums writes 6 fp64 local sums (sum and sum of squares, per
 * channel, of the quantities LAB is affine in: f_y, f_x - f_y, f_y - f_z; opaque to the caller) -> all-reduce(SUM) -> sx_reinhard_apply normalises with the global sums over
 * n_total_pixels = pixels per channel over all ranks. */
int sx_reinhard_sums(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                     double* sums_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_reinhard_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                      int64_t width, const double* sums_dev, double n_total_pixels, const float* ref_mean_dev,
                      const float* ref_std_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Per-tile source statistics (an extension: the reference pools over the batch; torchstain, tiatoolbox and HistomicsTK normalise ONE
 * image with its own statistics).  A batch of tiles from different slides is normalised tile by tile in two streaming launches, and a
 * tile's output does not depend on its neighbours in the batch.
 *
 * sx_reinhard_tile_stats: LAB mean and unbiased standard deviation of EVERY tile in one statistics pass (the tile's last arrival
 *   finishes the tile, in a fixed order).  tile_mean_out_dev, tile_std_out_dev: N x 3 floats each.  A tile of one pixel has std NaN.
 * sx_reinhard_transform_tiles: that pass, then the apply pass with every tile's OWN statistics.  tile_mean_out_dev / tile_std_out_dev
 *   receive them (both or neither; exactly one NULL is SX_ERR_BAD_ARG).  Two streaming launches and the clearing launch of the plain
 *   pooled call: any workspace contents are accepted, and a workspace that was READY is left ready, so the call may alternate with
 *   sx_reinhard_transform_ready on one workspace.
 * Both need sx_reinhard_tiles_workspace_bytes() bytes (at least the pooled size; for float32 with room for the 8-bit codes -- a call
 * on a workspace without that room runs without them, same bits).
 *
 * sx_reinhard_apply_stats: normalise with GIVEN source statistics -- ONE kernel launch on `stream`, nothing else enqueued, no
 *   workspace: a pixel is read, a pixel is written.
 *   source_mean_dev, source_std_dev   n_sources x 3 floats each (LAB on the reference's 0..255 scale, as sx_reinhard_fit writes them)
 *   n_sources                         1 (a slide's statistics for the whole batch) or n_tiles (row t serves tile t); anything else is
 *                                     SX_ERR_BAD_ARG
 *   The statistics and the reference are DEVICE memory read by the kernel (a captured graph replayed after new values were written
 *   into the same buffers uses the new values).  The arithmetic per pixel is the pooled apply pass's, a function of the float32
 *   statistics: sx_reinhard_fit's outputs with n_sources = 1 give the bits of sx_reinhard_transform, sx_reinhard_tile_stats' outputs
 *   with n_sources = n_tiles those of sx_reinhard_transform_tiles.
 *   Verified parameter domain (tests/_param_sweep.py): the bound of 1e-4 on [0, 1] against float64 is verified for finite
 *   statistics with ref_std / source_std in [0.1, 2.5] for L, a and b and a source mean in [-64, 320]; at a ratio of 5 the float32
 *   arithmetic of the reference itself is 6.5e-5 from float64.  Outside it every output element is finite and inside [0, 1]. */
size_t sx_reinhard_tiles_workspace_bytes(int dtype, int64_t n_tiles, int64_t height, int64_t width);
int sx_reinhard_tile_stats(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                           float* tile_mean_out_dev, float* tile_std_out_dev, void* workspace_dev, size_t workspace_bytes,
                           void* stream);
int sx_reinhard_transform_tiles(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                                int64_t width, const float* ref_mean_dev, const float* ref_std_dev,
                                float* tile_mean_out_dev, float* tile_std_out_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream);
int sx_reinhard_apply_stats(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                            int64_t width, const float* source_mean_dev, const float* source_std_dev, int64_t n_sources,
                            const float* ref_mean_dev, const float* ref_std_dev, void* stream);

/* ---------------------------------------------------------------- Histogram matching -------------
 * Replaces stainx_cuda_torch.histogram_matching (bindings.cpp:31) with the numerics of
 * HistogramMatchingTorch (torch_backend.py:134-301).  `channels_last` != 0: images are (N,H,W,3).
 *   ref_hist_dev  3 x 256 floats (per-channel normalised reference histograms)
 *   sx_hm_fit writes those; sx_hm_transform also leaves the pooled integer source histogram
 *   (3 x 256 uint32) and the float LUT (3 x 256) at the start of the workspace for inspection. */
size_t sx_hm_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
int sx_hm_fit(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
              int channels_last, float* hist_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_hm_transform(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                    int64_t width, int channels_last, const float* ref_hist_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);

/* The same three calls for a workspace in the READY state: zero-filled once by sx_hm_workspace_init() (or by the caller), and since then
 * only touched by completed calls of this section -- each of them leaves the workspace ready again (the kernel that reads the
 * histogram counters writes zeros back).  They skip the clearing launch in front of the histogram pass (~5 us of a 115 us call on
 * 64 x 3 x 1024 x 1024 uint8).  The plain calls above accept ANY workspace contents and leave it ready as well.  A *_ready transform
 * on a workspace that was not ready is noticed on the device (its counters do not add up to the pixels counted): bit 0 of the uint32
 * at byte sx_hm_workspace_status_offset() of the workspace is set and stays set until sx_hm_workspace_init(); the output of such a
 * call is not to be used.  No reference counterpart: the reference allocates its histogram inside every call
 * (torch_backend.py:139, histogram_matching.cu:49-81). */
int sx_hm_workspace_init(void* workspace_dev, size_t workspace_bytes, void* stream);
size_t sx_hm_workspace_status_offset(void);
#ifdef SX_DIAG
/* Diagnostic build: planar uint8 batches of at least 32 MB take the transform entry points above in ONE launch (workgroups keep part of the batch in
 * registers between counting and applying: same bits, measured slower than the two kernels -- DESIGN.md section 5; SX_HM_RESIDENT=0 in the
 * environment switches it off).  The uint32 at byte sx_hm_workspace_parity_offset() of the workspace toggles with every call that took
 * that form; sx_debug_hm_stamp_offset(): its phase stamps. */
size_t sx_hm_workspace_parity_offset(void);
size_t sx_debug_hm_stamp_offset(void);
#endif
int sx_hm_fit_ready(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                    int channels_last, float* hist_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_hm_transform_ready(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                          int64_t width, int channels_last, const float* ref_hist_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
int sx_hm_counts_ready(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                       int channels_last, unsigned long long* counts_out_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);

/* Source histogram pooled across ranks: sx_hm_counts writes the local 3 x 256 u64 counts -> all-reduce(SUM)
 * -> sx_hm_apply builds the LUT from the global counts (n_total_pixels per channel over all ranks). */
int sx_hm_counts(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                 int channels_last, unsigned long long* counts_out_dev, void* workspace_dev,
                 size_t workspace_bytes, void* stream);
int sx_hm_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                int channels_last, const unsigned long long* counts_dev, double n_total_pixels,
                const float* ref_hist_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* One histogram and one LUT per TILE against the one reference (an extension: the reference pools the source histogram over the
 * batch; scikit-image's match_histograms, tiatoolbox and HistomicsTK match ONE image).  Three launches and one clear whatever
 * n_tiles is: histogram pass into a 3 x 256 set of integer counters per tile, 3 x n_tiles LUT workgroups (the pooled LUT arithmetic,
 * with the tile's pixels), apply pass with the tile's own LUT.  Tile t's output is bit for bit sx_hm_transform of tile t alone.
 *   tile_counts_out_dev  n_tiles x 3 x 256 uint32, the histograms as counted; may be NULL
 *   tile_lut_out_dev     n_tiles x 3 x 256 floats, the float LUTs; may be NULL
 * The workspace needs sx_hm_tiles_workspace_bytes() bytes (the pooled Tables first: the status word lies where
 * sx_hm_workspace_status_offset() says).  Any workspace contents are accepted; the call leaves the workspace READY. */
size_t sx_hm_tiles_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
int sx_hm_transform_tiles(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                          int channels_last, const float* ref_hist_dev, uint32_t* tile_counts_out_dev,
                          float* tile_lut_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- Tissue masks ---------------------
 * An extension for Reinhard and histogram matching (HistomicsTK's reinhard(mask_out=), staintools' LuminosityThresholdTissueLocator,
 * tiatoolbox): statistics -- LAB mean / standard deviation, histograms -- over TISSUE pixels only, and background pixels written with
 * the bits of the input.  The unmasked entry points above are untouched.  Everywhere below:
 *   mask_dev               const uint8_t, n_tiles x height x width, non-zero = tissue (one value per pixel: a pixel's three channels are
 *                          in or out together), or NULL: the rule
 *   luminosity_threshold   the rule: a pixel is tissue iff L* / 100 < luminosity_threshold (0.8: staintools' and tiatoolbox's default),
 *                          L* of the pixel's unit value (u8 / 255, floats as they are) by the Reinhard section's colour conversion
 *                          (0.8 <-> 204 on its 0..255 scale).  L* is monotone in the linear-light luminance Y, so every kernel compares
 *                          Y with one constant derived on the host, by ONE device function: all entry points agree on every pixel.
 *                          Outside (0, 1) -- NaN included -- is SX_ERR_BAD_ARG; not read when mask_dev is given.
 * A tile (or pooled batch) with fewer than two tissue pixels has no statistics: mean and standard deviation NaN, and every apply pass
 * copies a tile through whose row of statistics holds a NaN.  The tissue edge is a hard edge: no smoothing.
 *
 * sx_tissue_mask: the rule as a call of its own, one streaming pass (and a clear of the counts).  mask_out_dev: n_tiles x height x
 *   width bytes, 1 / 0; tile_counts_out_dev: n_tiles uint64 tissue pixels per tile; either may be NULL, not both.  channels_last != 0:
 *   images are (N,H,W,3). */
int sx_tissue_mask(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                   double luminosity_threshold, uint8_t* mask_out_dev, unsigned long long* tile_counts_out_dev, void* stream);

/* ---- Tissue detection: a threshold taken from the data, and a clean-up of the mask -------------------
 * What staintools', tiatoolbox's and HistomicsTK's users do before an estimate: an Otsu threshold on the lightness, then a morphological
 * opening and closing of the mask.  Three device calls; the Otsu arithmetic itself is exact integer work on 256 counts per row and
 * stays with the caller (stainx_amd.otsu_threshold).
 *
 * sx_luminosity_histogram: 256-bin integer histograms of lightness, one memset and one streaming launch.  counts_out_dev: rows x 256
 *   uint64, rows = n_tiles, or 1 with pooled != 0 (required).  The bins are defined by the rule itself: with
 *   cut[k] = sx_tissue_y_cut of k / 256, k = 1..255, a pixel's bin is the number of k with !(Y < cut[k]), Y the luminance every masked
 *   kernel compares.  So the sum of bins 0..k-1 is EXACTLY the tissue count of sx_tissue_mask at luminosity_threshold = k / 256, for every
 *   k, element type and layout; a NaN pixel lands in bin 255 (background at every threshold).  Arguments as sx_tissue_mask.
 * sx_tissue_y_cut: host only.  The constant sx_tissue_mask derives from its threshold (a pixel is tissue iff Y < it); NaN for a
 *   threshold outside (0, 1).  Strictly increasing over k / 256.
 * sx_tissue_mask_tiles: sx_tissue_mask with a constant per tile.  tile_y_cut_dev: n_tiles floats in DEVICE memory read by the kernel (a
 *   captured call replayed after new cuts were written uses them; NULL is SX_ERR_BAD_ARG); tile i is tissue where Y < tile_y_cut_dev[i],
 *   and a NaN cut makes the whole tile background with count 0.  With every entry equal to the value sx_tissue_y_cut gives for t, mask
 *   and counts are the bits of sx_tissue_mask at t.  One launch and the clear of the counts. */
int sx_luminosity_histogram(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                            int pooled, unsigned long long* counts_out_dev, void* stream);
float sx_tissue_y_cut(double luminosity_threshold);
int sx_tissue_mask_tiles(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                         const float* tile_y_cut_dev, uint8_t* mask_out_dev, unsigned long long* tile_counts_out_dev, void* stream);

/* sx_mask_morphology: binary erosion, dilation, opening (erode, then dilate) and closing (dilate, then erode) of masks.
 *   mask_in_dev    n_tiles x height x width bytes, non-zero = set;   mask_out_dev: the same shape, 1 / 0.  mask_out_dev == mask_in_dev
 *                  is SX_ERR_BAD_ARG (not in place).
 *   element        SX_ELEMENT_SQUARE: the (2r+1) x (2r+1) box; SX_ELEMENT_DISK: the offsets with dx^2 + dy^2 <= r^2 (scikit-image's disk(r))
 *   radius         1 .. SX_MORPH_MAX_RADIUS; anything else is SX_ERR_BAD_ARG
 *   scratch_dev    n_tiles x height x width bytes for SX_MORPH_OPEN / SX_MORPH_CLOSE (NULL, mask_in_dev or mask_out_dev there:
 *                  SX_ERR_BAD_ARG); not read by erode / dilate, may be NULL
 *   tile_counts_out_dev   n_tiles uint64, the set pixels of the result per tile; may be NULL
 * Borders (OpenCV's default; scipy's binary_erosion(border_value=1) / binary_dilation(border_value=0)): what lies outside a tile never
 * constrains the result -- erosion reads it as set, dilation as unset -- so tissue that touches a tile's edge is not eaten from the
 * edge.  Tiles are independent.  One launch for erode / dilate, two for open / close, and the clear of the counts; every launch stages
 * its pixels with their halo on chip once, a bit per pixel. */
#define SX_MORPH_ERODE 0
#define SX_MORPH_DILATE 1
#define SX_MORPH_OPEN 2
#define SX_MORPH_CLOSE 3
#define SX_ELEMENT_SQUARE 0
#define SX_ELEMENT_DISK 1
#define SX_MORPH_MAX_RADIUS 31
int sx_mask_morphology(const uint8_t* mask_in_dev, uint8_t* mask_out_dev, int64_t n_tiles, int64_t height, int64_t width, int op,
                       int element, int radius, uint8_t* scratch_dev, unsigned long long* tile_counts_out_dev, void* stream);

/* ---- Mask components: labelling and area filters ------------------------------------------------------
 * What morphology cannot do: remove objects, and fill holes, BY AREA (tiatoolbox's MorphologicalMasker min_region_size, the object and
 * hole filters of HistomicsTK- and CLAM-style pipelines, scikit-image's remove_small_objects / remove_small_holes on the Otsu mask).
 * Masks as sx_mask_morphology takes them: n_tiles x height x width bytes, non-zero = set; tiles are independent, nothing outside a
 * tile belongs to a component and no component continues into the next tile.
 *   connectivity   4: the edge neighbours (scipy's generate_binary_structure(2, 1), scikit-image's connectivity=1); 8: the diagonals
 *                  too (np.ones((3, 3)), connectivity=2, OpenCV's default).  Anything else is SX_ERR_BAD_ARG.
 *   label          of a set pixel: 1 + (y * width + x) of the FIRST pixel of its component in raster order, within its tile; 0 of an
 *                  unset pixel.  A function of the mask alone (scipy.ndimage.label, canonicalised).  int32: height x width must not
 *                  exceed 2^31 - 2 (SX_ERR_BAD_ARG).
 *
 * sx_mask_components: replaces scipy.ndimage.label / skimage.measure.label + np.bincount on the host.
 *   invert                   != 0: the components of the COMPLEMENT are labelled (the "holes": a background region that touches the
 *                            tile's edge is one of them)
 *   labels_out_dev           n_tiles x height x width int32 (required)
 *   areas_out_dev            the same shape, int32: at a component's first pixel its pixel count, 0 everywhere else; may be NULL
 *   tile_components_out_dev  n_tiles uint64, the components per tile; may be NULL
 *   Three launches (two where a tile is one block of 256 x 64) and the clear of the counts; no workspace.
 * sx_mask_area_filter: replaces skimage.morphology.remove_small_objects (holes == 0) and remove_small_holes (holes != 0).
 *   holes == 0: every set pixel whose component has fewer than min_area pixels is cleared (an area equal to min_area stays);
 *   holes != 0: every unset pixel whose component OF THE COMPLEMENT has fewer than min_area pixels is set -- scikit-image's rule, under
 *   which glass that touches the tile's edge counts as a hole: choose min_area below a tile's glass.  Bit for bit
 *   holes(m) == 1 - objects(1 - m).
 *   mask_out_dev         n_tiles x height x width bytes, 1 / 0; must be neither mask_in_dev nor inside the workspace (SX_ERR_BAD_ARG)
 *   min_area             at least 1 (SX_ERR_BAD_ARG below); 1 gives the mask's own bits as 1 / 0; above height x width everything is
 *                        removed (filled)
 *   workspace_dev        sx_mask_components_workspace_bytes() bytes, any contents
 *   tile_counts_out_dev  n_tiles uint64, the set pixels of the result per tile; may be NULL
 *   The launches of sx_mask_components, one pixel-local launch and the clear of the counts.
 * sx_mask_components_workspace_bytes: host only; 0 for non-positive sizes, 8 bytes per pixel (labels and areas) and room to align. */
size_t sx_mask_components_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
int sx_mask_components(const uint8_t* mask_in_dev, int64_t n_tiles, int64_t height, int64_t width, int connectivity, int invert,
                       int32_t* labels_out_dev, int32_t* areas_out_dev, unsigned long long* tile_components_out_dev, void* stream);
int sx_mask_area_filter(const uint8_t* mask_in_dev, uint8_t* mask_out_dev, int64_t n_tiles, int64_t height, int64_t width,
                        int connectivity, int holes, int64_t min_area, void* workspace_dev, unsigned long long* tile_counts_out_dev,
                        void* stream);

/* ---- Saturation-channel tissue detection: saturation maps, a median filter, level histograms and thresholds ----
 * The front half of CLAM's segmentTissue: threshold the HSV saturation ("is the pixel coloured") after a median filter, where the
 * luminosity rule asks "is the pixel dark".  A grey pixel -- shadow, coverslip edge, colourless dust -- has saturation 0.  Every result
 * is an integer and every definition exact.  Level maps are n_tiles x height x width bytes; tiles are independent.
 *
 * The 8-bit level of a stored element: a uint8 element is its own level; any other type starts from its unit value v (float32; a
 *   double is rounded to float first) and the level is rintf(fminf(fmaxf(255.0f * v, 0.0f), 255.0f)): one float32 multiply, a clamp,
 *   round-half-even; +inf gives 255, -inf 0.  A u / 255 float32 or float64 tile has the levels of its uint8 original.  So has an
 *   f16 or bf16 tile rounded from u / 255, but bf16 only just: its rounding moves 255 v by up to 0.498 of a level, so any further
 *   arithmetic on a bf16 tile loses levels.
 * sx_saturation_map: levels_out_dev[pixel] = S, one streaming launch.  With M and m the largest and smallest of the pixel's three
 *   levels: S = 0 if M == 0, else (510 (M - m) + M) / (2 M) in integer division -- 255 (M - m) / M rounded half up, in 0..255.  A pixel
 *   with a NaN in any channel has S = 0 (background, as under the luminosity rule).  This is the library's own exact rule; it is not
 *   pinned to any other library's table-based conversion.  images_dev, dtype, channels_last as sx_tissue_mask; NULL pointers and
 *   non-positive sizes are SX_ERR_BAD_ARG, an unknown dtype SX_ERR_DTYPE.
 * sx_median_filter_u8: levels_out_dev[pixel] = the value of rank (size^2 + 1) / 2 among the size x size window centred on the pixel,
 *   the window read with replicated borders (cv2.medianBlur's border, scipy.ndimage.median_filter(mode="nearest")) inside the pixel's
 *   own tile.  On a 0 / 1 mask this is the majority filter.
 *   size             odd, 3 .. SX_MEDIAN_MAX_SIZE; anything else is SX_ERR_BAD_ARG
 *   levels_out_dev   must not be levels_in_dev (SX_ERR_BAD_ARG: not in place)
 *   One launch, no workspace, no synchronisation: a workgroup stages its 64 x 64 block with the halo on chip once, as eight bit planes.
 * sx_level_histogram: counts_out_dev[row][b] = the pixels of level b; rows = n_tiles, or 1 with pooled != 0.  rows x 256 uint64
 *   (required).  One memset and one launch.
 * sx_level_mask_tiles: mask_out_dev = 1 where level > tile_thresholds_dev[tile], else 0 (cv2's THRESH_BINARY, CLAM's sthresh).
 *   tile_thresholds_dev   n_tiles int32 in DEVICE memory read by the kernel (a captured call replayed after new thresholds were
 *                         written uses them; NULL is SX_ERR_BAD_ARG).  A negative threshold sets the whole tile, one >= 255 clears it.
 *   mask_out_dev, tile_counts_out_dev (n_tiles uint64 set pixels per tile): either may be NULL, not both.
 *   One launch and the clear of the counts. */
#define SX_MEDIAN_MAX_SIZE 15
int sx_saturation_map(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                      uint8_t* levels_out_dev, void* stream);
int sx_median_filter_u8(const uint8_t* levels_in_dev, uint8_t* levels_out_dev, int64_t n_tiles, int64_t height, int64_t width, int size,
                        void* stream);
int sx_level_histogram(const uint8_t* levels_dev, int64_t n_tiles, int64_t height, int64_t width, int pooled,
                       unsigned long long* counts_out_dev, void* stream);
int sx_level_mask_tiles(const uint8_t* levels_dev, int64_t n_tiles, int64_t height, int64_t width, const int32_t* tile_thresholds_dev,
                        uint8_t* mask_out_dev, unsigned long long* tile_counts_out_dev, void* stream);

/* ---- Focus measurement: grey maps, Laplacian variance and Tenengrad as integer sums, cell grids as pixel masks ----
 * The focus filter that HistoQC-, CLAM- and tiatoolbox-style pipelines run between "find the tissue" and "estimate the stain".  The
 * score is a ratio of integer sums, so the sums are the result: exact, independent of the order of adding, and poolable over batches,
 * slides and ranks.  images_dev, dtype, channels_last as sx_tissue_mask; NULL pointers and non-positive sizes are SX_ERR_BAD_ARG, an
 * unknown dtype SX_ERR_DTYPE; a refused call writes nothing.
 *
 * The grey level of a pixel with 8-bit levels r, g, b (the level rule of the saturation section above):
 *   Y = (4899 r + 9617 g + 1868 b + 8192) >> 14, in 0..255 (the weights sum to 16384): the fixed-point rule of an 8-bit RGB -> grey
 *   conversion.  A pixel with a NaN in any channel has Y = 0.
 * The stencils on Y, per tile, in int32, the border reflected without repeating the edge (-1 -> 1, H -> H - 2; an axis of length 1 maps
 *   to 0: OpenCV's BORDER_REFLECT_101, scipy's mode="mirror", numpy's pad mode "reflect"); tiles never see each other:
 *   L = Y[y-1,x] + Y[y+1,x] + Y[y,x-1] + Y[y,x+1] - 4 Y[y,x]  (cv2.Laplacian with ksize = 1), |L| <= 1020;
 *   Gx, Gy the 3 x 3 Sobel responses ([1 2 1] smoothing, [-1 0 1] derivative), T = Gx^2 + Gy^2 <= 2 080 800.
 * sx_grey_map: levels_out_dev[pixel] = Y, n_tiles x height x width bytes, one streaming launch.  It replaces a float RGB -> grey
 *   conversion in torch or cv2.cvtColor on the CPU; sx_median_filter_u8, sx_level_histogram and sx_level_mask_tiles take its output.
 * sx_focus_statistics / sx_focus_statistics_masked: statistics_out_dev = four planes of int64 words, in this order: pixels, sum L
 *   (signed), sum L^2, sum T; a plane holds one word per cell, n_tiles x grid_h x grid_w.  It replaces cv2.Laplacian(gray,
 *   CV_64F).var() per tile on the CPU, or a float conv2d and var() in torch with their temporaries.
 *   block_h, block_w   the cell: 0, 0 is the whole tile (grid 1 x 1); otherwise each side is 8, 16, 32, 64 or a multiple of 64 and the
 *                      grid is ceil(height / block_h) x ceil(width / block_w), edge cells partial.  Anything else is SX_ERR_BAD_ARG.
 *   pooled             != 0: one cell for the whole batch (each plane one word); with block 0, 0 only, else SX_ERR_BAD_ARG.
 *   mask_dev           (the masked twin) n_tiles x height x width bytes: a pixel enters its cell iff its byte is non-zero; neighbours
 *                      are read whatever their bytes say.  NULL is SX_ERR_BAD_ARG.  Without a mask every pixel enters.
 *   One launch that reads the tile once and writes nothing but the words.  Cells with both sides <= 64 are written with plain
 *   stores; larger cells (the whole tile, the batch) take 64-bit integer adds into words cleared first: a memset, or a clearing
 *   launch while the stream is being captured.  No floating-point atomics, no workspace, no synchronisation.
 * sx_cells_mask: mask_out_dev[tile][y][x] = 1 iff cells_dev[tile][y / block_h][x / block_w] != 0 and (mask_dev given) the pixel's
 *   mask byte != 0, else 0; tile_counts_out_dev the set pixels per tile (n_tiles uint64).  It replaces np.repeat / F.interpolate of a
 *   cell grid and the AND with a tissue mask.  cells_dev is n_tiles x grid_h x grid_w bytes, the grid as above (block sides as
 *   above, no 0); mask_dev may be NULL; mask_out_dev, tile_counts_out_dev: either may be NULL, not both.  One streaming launch and
 *   the clear of the counts. */
int sx_grey_map(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                uint8_t* levels_out_dev, void* stream);
int sx_focus_statistics(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                        int64_t block_h, int64_t block_w, int pooled, long long* statistics_out_dev, void* stream);
int sx_focus_statistics_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                               int64_t block_h, int64_t block_w, int pooled, const unsigned char* mask_dev,
                               long long* statistics_out_dev, void* stream);
int sx_cells_mask(const uint8_t* cells_dev, int64_t n_tiles, int64_t height, int64_t width, int64_t block_h, int64_t block_w,
                  const unsigned char* mask_dev, uint8_t* mask_out_dev, unsigned long long* tile_counts_out_dev, void* stream);

/* Reinhard.  per_tile != 0: every tile its own statistics (N rows, a tile's result does not depend on its neighbours); per_tile == 0: one
 * set pooled over the tissue of the whole batch (one row).  Workspace: sx_reinhard_masked_workspace_bytes(); any contents are accepted
 * and a workspace that was READY (sx_reinhard_transform_ready) is left ready, so the calls may alternate with that one and with
 * sx_reinhard_transform_tiles on one workspace.
 * sx_reinhard_stats_masked: the statistics pass alone.  mean_out_dev, std_out_dev: rows x 3 floats (required); counts_out_dev: rows
 *   uint64 tissue pixels, may be NULL.  With every pixel tissue the rows are bit for bit those of sx_reinhard_tile_stats /
 *   sx_reinhard_fit (same grid, same reduction order; the divisor is the exact integer count).
 * sx_reinhard_transform_masked: that pass, then the apply pass: two streaming launches and the clearing launch.  mean_out_dev /
 *   std_out_dev: both or neither (exactly one NULL is SX_ERR_BAD_ARG); counts_out_dev may be NULL.
 * sx_reinhard_apply_stats_masked: sx_reinhard_apply_stats with a mask -- ONE launch on `stream`, nothing else enqueued, no workspace;
 *   statistics, reference and mask are DEVICE memory read by the kernel (a captured graph replayed after new values were written into
 *   the same buffers uses the new values).  A tissue pixel gets exactly the bits the unmasked apply pass gives with those statistics. */
size_t sx_reinhard_masked_workspace_bytes(int dtype, int64_t n_tiles, int64_t height, int64_t width);
int sx_reinhard_stats_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                             const uint8_t* mask_dev, double luminosity_threshold, int per_tile, float* mean_out_dev,
                             float* std_out_dev, unsigned long long* counts_out_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream);
int sx_reinhard_transform_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                                 int64_t width, const float* ref_mean_dev, const float* ref_std_dev, const uint8_t* mask_dev,
                                 double luminosity_threshold, int per_tile, float* mean_out_dev, float* std_out_dev,
                                 unsigned long long* counts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_reinhard_apply_stats_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                                   int64_t width, const float* source_mean_dev, const float* source_std_dev, int64_t n_sources,
                                   const float* ref_mean_dev, const float* ref_std_dev, const uint8_t* mask_dev,
                                   double luminosity_threshold, void* stream);

/* A TARGET PER TILE (an extension: statistics-space augmentation -- RandStainNA, Shen et al. 2022 --, Reinhard to per-tile or per-slide
 * targets without a fit).
 * sx_reinhard_apply_targets: sx_reinhard_apply_stats with n_targets rows of target statistics -- ONE kernel launch on `stream`, nothing
 *   else enqueued, no workspace.
 *   source_mean_dev, source_std_dev   n_sources x 3 floats each, n_sources = 1 or n_tiles (row t serves tile t)
 *   target_mean_dev, target_std_dev   n_targets x 3 floats each, n_targets = 1 or n_tiles (row t serves tile t)
 *   Any other n_sources / n_targets is SX_ERR_BAD_ARG.  All four arrays are DEVICE memory read by the kernel (a captured graph replayed
 *   after new values were written into the same buffers uses the new values).  The arithmetic is the one body of the apply pass: with
 *   n_targets = 1 and finite rows the output is bit for bit sx_reinhard_apply_stats', and tile t of a batched call is the one-tile call
 *   with rows t.  If any of a tile's source or target rows holds a NaN the tile is copied with the bits of its input (tiles of fewer than
 *   two pixels or tissue pixels, explicit "leave this tile" rows); sx_reinhard_apply_stats(_masked) keep their behaviour on such rows.
 * sx_reinhard_apply_targets_masked: the same with a mask, with the semantics of sx_reinhard_apply_stats_masked (mask_dev: (N, H, W)
 *   bytes, or NULL for the luminosity rule with luminosity_threshold in (0, 1)): a tissue pixel gets the bits of the unmasked call, a
 *   background pixel the bits of its input. */
int sx_reinhard_apply_targets(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                              int64_t width, const float* source_mean_dev, const float* source_std_dev, int64_t n_sources,
                              const float* target_mean_dev, const float* target_std_dev, int64_t n_targets, void* stream);
int sx_reinhard_apply_targets_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height,
                                     int64_t width, const float* source_mean_dev, const float* source_std_dev, int64_t n_sources,
                                     const float* target_mean_dev, const float* target_std_dev, int64_t n_targets,
                                     const uint8_t* mask_dev, double luminosity_threshold, void* stream);

/* Histogram matching, NCHW and NHWC.  The three 256-bin histograms count tissue pixels only, and the LUT arithmetic takes the TISSUE count
 * as its number of pixels (the sum of a channel's histogram); a tissue pixel gets its LUT value, a background pixel the bits of its
 * input (floats are not quantised).  Pixel-wise kernels: each pass reads the pixels (and the mask, where one is given) and nothing
 * else.  One clear, the histogram pass, the LUT launch, the apply pass.  Workspace: sx_hm_masked_workspace_bytes(); any contents are
 * accepted and the workspace is left READY (the status word lies where sx_hm_workspace_status_offset says: bit 0 is set when a
 * channel's total does not agree with the tissue pixels counted).
 * sx_hm_fit_masked: the normalised tissue histograms of the whole batch, 3 x 256 floats; tissue_count_out_dev: one uint64, may be NULL.
 * sx_hm_transform_masked: per_tile != 0: one histogram and one LUT per tile (sets = n_tiles); per_tile == 0: one pooled over the tissue
 *   of the batch (sets = 1).  tile_counts_out_dev: sets x 3 x 256 uint32 histograms as counted; tile_lut_out_dev: sets x 3 x 256 floats;
 *   tissue_counts_out_dev: sets uint64; each may be NULL. */
size_t sx_hm_masked_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
int sx_hm_fit_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                     const uint8_t* mask_dev, double luminosity_threshold, float* hist_out_dev,
                     unsigned long long* tissue_count_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_hm_transform_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                           int channels_last, const float* ref_hist_dev, const uint8_t* mask_dev, double luminosity_threshold,
                           int per_tile, uint32_t* tile_counts_out_dev, float* tile_lut_out_dev,
                           unsigned long long* tissue_counts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- Histogram matching, slide level ----
 * An extension: ESTIMATE the integer histograms of a source once (a thumbnail, a sample of tissue tiles, many batches), build lookup
 * tables from GIVEN counts, APPLY given tables to every tile of the slide.  Histograms are integer counts: those of different batches,
 * slides or ranks add up exactly (add the uint64 tensors), and a table built from added counts is bit for bit the table of the
 * concatenated pixels.
 *
 * sx_hm_estimate / sx_hm_estimate_masked: the histogram pass of the calls above as a call of its own.  per_tile != 0: one set per tile
 *   (sets = n_tiles); per_tile == 0: one set pooled over the batch (sets = 1).  The masked form counts tissue pixels only (mask_dev /
 *   luminosity_threshold as in the tissue-mask section).
 *   counts_out_dev  sets x 3 x 256 uint64: bin b of channel c; unmasked, the bincount of the tile's (batch's) grey levels; masked, the
 *                   tile_counts_out of sx_hm_transform_masked with the same arguments
 *   pixels_out_dev  sets uint64: the pixels (tissue pixels) counted per channel; may be NULL
 *   Workspace: sx_hm_tiles_workspace_bytes() / sx_hm_masked_workspace_bytes(); any contents are accepted and the workspace is left READY,
 *   so the calls may alternate with sx_hm_transform_ready, sx_hm_transform_tiles and sx_hm_transform_masked on one workspace.
 * sx_hm_tables: float lookup tables from GIVEN counts: one launch of 3 x n_sets workgroups, no workspace.
 *   counts_dev   n_sets x 3 x 256 uint64;  pixels_dev  n_sets uint64, DEVICE memory, required: the divisor of set s
 *   lut_out_dev  n_sets x 3 x 256 floats.  The arithmetic of the LUT launch of sx_hm_transform: count / float(pixels + 1e-8), running sums
 *   in torch.cumsum's order.  A set with pixels == 0 gets the IDENTITY table (entry b = b): a source without tissue leaves grey levels
 *   where they are.  (The reference never meets zero pixels; its arithmetic would give a table of zeros, i.e. black.)
 * sx_hm_apply_tables / sx_hm_apply_tables_masked: the apply pass with GIVEN tables -- ONE launch on `stream`, nothing else enqueued, no
 *   workspace.  lut_dev: n_sources x 3 x 256 floats (0..255, what sx_hm_tables writes), DEVICE memory read by the kernel: a captured
 *   graph replayed after new tables (or mask bytes) were written into the same buffers uses the new values.  n_sources is 1 (one
 *   table set for the batch) or n_tiles (set t serves tile t); anything else is SX_ERR_BAD_ARG.  Every workgroup converts its source's
 *   tables to the output element on the way into LDS.  Masked: a tissue pixel gets exactly the bits of the unmasked call, a
 *   background pixel the bits of its input (floats are not quantised).
 *   Table entries need not lie inside 0..255 (given tables may be blended or edited ones): for EVERY output type an entry is clamped to
 *   [0, 255] first and a NaN entry is 0 -- uint8: trunc(clamp(v, 0, 255)), so 255.5, 256, 1e9 and +Inf give 255, -0.5, -1 and -Inf give 0;
 *   floats: clamp(v / 255, 0, 1).  Tables inside 0..255 (all that sx_hm_tables writes) give the bits they always gave. */
int sx_hm_estimate(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last, int per_tile,
                   unsigned long long* counts_out_dev, unsigned long long* pixels_out_dev, void* workspace_dev,
                   size_t workspace_bytes, void* stream);
int sx_hm_estimate_masked(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                          int per_tile, const uint8_t* mask_dev, double luminosity_threshold, unsigned long long* counts_out_dev,
                          unsigned long long* pixels_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_hm_tables(const unsigned long long* counts_dev, const unsigned long long* pixels_dev, int64_t n_sets, const float* ref_hist_dev,
                 float* lut_out_dev, void* stream);
int sx_hm_apply_tables(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                       int channels_last, const float* lut_dev, int64_t n_sources, void* stream);
int sx_hm_apply_tables_masked(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                              int channels_last, const float* lut_dev, int64_t n_sources, const uint8_t* mask_dev,
                              double luminosity_threshold, void* stream);

/* ---------------------------------------------------------------- Vahadane -----------------------
 * The other H&E estimator (Vahadane et al. 2016; staintools, tiatoolbox): sparse non-negative matrix factorisation of the optical
 * density with two atoms.  An extension: the reference has no counterpart.  What the calls write is a stain basis and its maximal
 * concentrations in sx_macenko_estimate's layout, so sx_macenko_apply(_masked) and sx_macenko_separate_apply(_masked) take them as they are.
 *
 * A GROUP is a tile, or with pooled != 0 the whole batch (rows = n_tiles, or 1).  S is the group's masked-in pixels (mask_dev: one
 * byte per pixel, (N, H*W), non-zero = in, sx_tissue_mask's layout; NULL: every pixel).  V (3,|S|) is the optical density of the
 * transform, -log((level + 1) / 240).  Values under masked-out pixels never matter, NaN included; a non-finite masked-in pixel makes
 * the group's result undefined.  Images are planar (N,3,H,W) of any of the five element types.
 *
 * sx_vahadane_estimate minimises 0.5 |V - W H|^2 + lambda |H|_1 over W (3,2) >= 0 with unit columns and H (2,|S|) >= 0 by exactly
 * `iterations` rounds (1..1000, no early exit: nothing synchronises, the call can be captured, two calls give the same bits):
 *   coding step      per pixel, float32, from the float32 rounding of W: with g = w1.w2, b = W^T v - lambda, d = 1 - g^2 the
 *                    candidate h = ((b1 - g b2)/d, (b2 - g b1)/d) if both components are > 0 (and d > 1e-6); else (b1, 0) if b1 > 0
 *                    and b2 - g b1 <= 0; else (0, b2) if b2 > 0; else (0, 0) -- the exact two-variable non-negative lasso
 *   dictionary step  per group, fp64, from A = H H^T and B = V H^T: for j = 0, 1: u = W[:,j] + (B[:,j] - W A[:,j]) / A[j,j],
 *                    u = max(u, 0), W[:,j] = u / |u|; an atom with A[j,j] == 0 or |u| == 0 keeps its column
 * and then, if W[0,0] < W[0,1], swaps the columns (haematoxylin: the larger red optical density) and rounds to float32.
 *   init_he_dev    n_init x 6 floats, (3,2) row-major, columns normalised on the device; n_init is 1 or rows
 *   lambda         >= 0, finite (staintools / tiatoolbox: 0.1)
 *   he_out_dev     rows x 6 floats; a group without a masked-in pixel gets NaN
 *   max_c_out_dev  rows x 2 floats, or NULL to skip them: what sx_stain_max_concentrations returns for he_out_dev
 *   pixels_out_dev rows uint64, or NULL: |S|, exact
 * Two launches per round (a streaming pass with fixed-order reductions, no floating-point atomics; one workgroup per group).  A tile's
 * row has the same bits alone or inside a batch, and a pooled estimate of a one-tile batch has the bits of that tile's row.
 *
 * sx_stain_max_concentrations: for GIVEN bases he_dev (n_sources x 6 floats; n_sources is 1 or rows) the two nearest-rank 99th
 * percentiles, k = 1 + round(0.01 * 99 * (|S| - 1)) half to even, over S of the float32 concentrations that
 * sx_macenko_separate_apply(_masked) writes in own-basis mode for that basis -- bit for bit.  An exact radix selection: a memset,
 * three streaming passes with integer histograms and three one-workgroup steps.  A group without a masked-in pixel gets NaN.
 *
 * flags: SX_MACENKO_CLASSIC (a no-op) only; anything else, SX_MACENKO_CHANNELS_LAST included, is SX_ERR_BAD_ARG.  Argument errors
 * (a NULL required pointer; n, h, w not positive or overflowing; iterations outside 1..1000; lambda negative or not finite; n_init /
 * n_sources other than 1 or rows: SX_ERR_BAD_ARG; an unknown element type: SX_ERR_DTYPE; a workspace smaller than
 * sx_vahadane_workspace_bytes() or misaligned: SX_ERR_WORKSPACE) are returned before anything is enqueued. */
size_t sx_vahadane_workspace_bytes(int dtype, int64_t n_tiles, int64_t height, int64_t width);
int sx_vahadane_estimate(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, const uint8_t* mask_dev,
                         int pooled, const float* init_he_dev, int64_t n_init, double lambda, int iterations, float* he_out_dev,
                         float* max_c_out_dev, unsigned long long* pixels_out_dev, unsigned flags, void* workspace_dev,
                         size_t workspace_bytes, void* stream);
int sx_stain_max_concentrations(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                                const uint8_t* mask_dev, int pooled, const float* he_dev, int64_t n_sources, float* max_c_out_dev,
                                unsigned long long* pixels_out_dev, unsigned flags, void* workspace_dev, size_t workspace_bytes,
                                void* stream);

/* ---------------------------------------------------------------- luminosity standardisation -----
 * staintools' LuminosityStandardizer.standardize, exact and on the device: take a percentile of the lightness L*, scale L* so that the
 * percentile becomes white, clip at white, leave a* and b* alone.  An extension: the reference has no counterpart.  Images are planar
 * (N,3,H,W) of any of the five element types.
 *
 * Y of a pixel is the float32 luminance sx_tissue_mask, sx_tissue_mask_tiles and sx_luminosity_histogram compare (the colour
 * conversion's middle row on the linear-light values; a double is rounded to float first).  L* is monotone in Y, so the percentile of
 * L* is L* of the percentile of Y and the selection runs on Y.
 *
 * sx_luminosity_percentile: a ROW is a tile, or with pooled != 0 the whole batch (rows = n_tiles, or 1).  S is the row's masked-in
 * pixels (mask_dev: one byte per pixel, (N, H*W), non-zero = in, sx_tissue_mask's layout; NULL: every pixel) whose Y is not NaN.  The
 * result is the nearest rank with the rule of sx_stain_max_concentrations, k = 1 + rint(0.01 * percentile * (|S| - 1)), half to even,
 * in doubles: the k-th smallest Y of S, a float32 that occurs in the data.  (Not numpy's method="nearest", and not staintools' linear
 * interpolation over 8-bit LAB.)
 *   percentile         in (0, 100], finite
 *   luminance_out_dev  rows floats; NaN for an empty S
 *   pixels_out_dev     rows uint64, or NULL: |S|, exact
 * An exact radix selection: a memset, three streaming passes with integer histograms and three one-workgroup steps on `stream`; no
 * floating-point atomics, no host synchronisation, the call can be captured.  A tile's row has the same bits alone or inside a batch,
 * and a pooled one-tile batch gives the bits of that tile's row.
 *
 * sx_luminosity_apply: ONE launch on `stream`, no workspace.  luminance_dev: n_sources floats in DEVICE memory read by the kernel
 * (n_sources is 1: row 0 for every tile, or n_tiles: row `tile`).  From the row's Y_p, in fp64: f_p = Y_p > 0.008856 ? cbrt(Y_p) :
 * 7.787 Y_p + 16/116, L_p = 116 f_p - 16, g = 100 / L_p.  Per pixel, in float32, with (f_x, f_y, f_z) of the LAB conversion:
 * f_y' = min(g f_y + (16/116)(1 - g), 1), f_x' = f_y' + (f_x - f_y), f_z' = f_y' - (f_y - f_z), and back to sRGB as
 * sx_reinhard_apply_stats goes: L*' = min(100 L* / L_p, 100), a* and b* unchanged, nothing quantised on the way.  A row that is NaN or
 * gives L_p <= 0 (a black tile) copies its tiles through bit for bit; so does a row that is exactly 1 (L_p = 100: the gain is 1 and the
 * map the identity on [0, 1], which the float32 round trip and the truncation to a level would not give back; members outside [0, 1]
 * are then kept, not clipped).  What a NaN pixel becomes is unspecified.  Not in place.
 * L_p is formed in fp64 as written above, so a positive Y_p below 1.8e-18 (every denormal) is absorbed by the 16/116 and gives L_p = 0
 * exactly: a black row, copied.  The smallest positive L_p is 3.6e-15 and the largest gain 2.8e16, a finite float32: g f_y + (16/116)(1 - g)
 * never meets Inf - Inf.  Verified parameter domain (tests/_param_sweep.py): the bound of 1e-4 on [0, 1] against float64 is
 * verified for finite rows with L_p >= 0.25 (a gain of 400; the cancellation in g f_y + (16/116)(1 - g) costs about g * 1e-8 on a dark
 * pixel) and |g - 1| >= 1e-3, or Y_p exactly 1: a row within a few float32 steps of 1 is NOT copied, runs the map at a gain that is 1 to
 * rounding, and on uint8 tiles may then come out one level off anywhere (every element lies within the bound of its own level).
 *
 * Argument errors (a NULL required pointer; n, h, w not positive or overflowing; a percentile outside (0, 100] or not finite;
 * n_sources other than 1 or n_tiles; out_dev == images_dev: SX_ERR_BAD_ARG; an unknown element type: SX_ERR_DTYPE; a workspace
 * smaller than sx_luminosity_workspace_bytes() or misaligned: SX_ERR_WORKSPACE) are returned before anything is enqueued. */
size_t sx_luminosity_workspace_bytes(int dtype, int64_t n_tiles, int64_t height, int64_t width);
int sx_luminosity_percentile(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, const uint8_t* mask_dev,
                             int pooled, double percentile, float* luminance_out_dev, unsigned long long* pixels_out_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
int sx_luminosity_apply(const void* images_dev, void* out_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                        const float* luminance_dev, int64_t n_sources, void* stream);
#ifdef SX_DIAG
/* Diagnostic build: sx_luminosity_percentile with one LDS add per pixel instead of one per run of equal bins -- same result; what the run
 * counting is measured against on glass. */
int sx_luminosity_percentile_plain(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width,
                                   const uint8_t* mask_dev, int pooled, double percentile, float* luminance_out_dev,
                                   unsigned long long* pixels_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
#endif

/* ---------------------------------------------------------------- tissue pixel sampling -----------
 * HistomicsTK's sample_pixels on the device, exact: from a batch and a mask, a fixed-shape tile of at most K masked-in pixels per
 * GROUP -- a tile, or with pooled != 0 the whole batch (groups = n_tiles, or 1) -- chosen by an integer rule and copied bit for bit, plus
 * a validity mask.  The result is an ordinary small planar tile with an explicit mask: every masked estimate above takes it as it is,
 * and samples of any number of batches, concatenated along the group axis, make one bounded pooled estimate of a slide.  An extension:
 * the reference has no counterpart.
 *
 * The rule.  A group's population is its masked-in pixels (mask_dev: one byte per pixel, (N, H*W), non-zero = in, the layout every
 * masked entry point reads; NULL: every pixel), ranked 0 .. n-1 in raster order, pooled: tile after tile in batch order.  K = sample_size;
 * the slots 0 .. K-1 are the pixels of the output tile in raster order.
 *   n <= K   slot r holds the pixel of rank r, valid = 1; the slots n .. K-1 hold zero bytes, valid = 0; offset is not used.
 *   n >  K   slot j holds the pixel of rank (j * n + o) div K with o = offset mod n, in 64-bit integers, valid = 1: the ranks are
 *            strictly increasing in j and the largest is below n.
 * A pixel is moved as its three values in the element type of the images -- no conversion: NaN payloads and -0.0 survive.
 *   images_dev          (N,3,H,W), or (N,H,W,3) with channels_last != 0, any of the five element types
 *   sample_size         1 .. 2^24
 *   offset              >= 0; another offset takes another sample of a group with n > K
 *   pixels_out_dev      groups x 3 x K elements of the images' type: ALWAYS planar, slot j of channel c of group g at (g * 3 + c) * K + j
 *   valid_out_dev       groups x K bytes, 1 / 0
 *   taken_out_dev       groups int32: min(n, K)
 *   population_out_dev  groups int64: n
 *   workspace_dev       sx_sample_workspace_bytes() bytes, 8-byte aligned; any contents
 * Three launches on `stream` -- chunk counts read from the mask with 16-byte loads, one workgroup per group for the prefix over the
 * chunks, the copy -- with every byte of the four outputs written by exactly one thread: no memset, no atomics, no workgroup that waits
 * for another, no host synchronisation; the call can be captured.  A group's row has the same bits alone or inside a batch.
 *
 * Errors, returned before anything is enqueued.  SX_ERR_BAD_ARG: a NULL required pointer (mask_dev may be NULL); n, h, w not positive
 * (a batch of zero tiles is the caller's to skip, as everywhere above); sample_size outside 1 .. 2^24; offset < 0; a group of 2^31
 * pixels or more; a workspace that is NULL, misaligned or smaller than the size query says.  SX_ERR_DTYPE: an unknown element type.
 * The size query returns 0 for sizes the call refuses. */
size_t sx_sample_workspace_bytes(int64_t n_tiles, int64_t height, int64_t width);
int sx_sample_pixels(const void* images_dev, int dtype, int64_t n_tiles, int64_t height, int64_t width, int channels_last,
                     const uint8_t* mask_dev, int pooled, int64_t sample_size, int64_t offset,
                     void* pixels_out_dev, uint8_t* valid_out_dev, int32_t* taken_out_dev, int64_t* population_out_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STAINX_HIP_H */
