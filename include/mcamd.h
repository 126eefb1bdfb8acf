/* mcamd.h -- C ABI of libmcamd.so, the MI355X (gfx950) hot path of
 * modelcompression_amd: YOLOv2/Darknet-19 convolution forward/backward and the
 * src/pruning mask kernels of AnishDelft/ModelCompression.
 *
 * The reference has no FFI layer: its operator API is
 * Python calling torch.  Each entry point below names the reference call site it
 * replaces.  Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no C++/torch types;
 *   - every pointer is a DEVICE pointer into memory owned by the caller
 *     (PyTorch-ROCm's allocator in practice); the library never allocates,
 *     frees or retains device memory -- workspaces are caller-provided and sized
 *     by the *_workspace_bytes queries;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     calls only enqueue work on it: no host synchronisation, graph-capturable;
 *   - returns 0 on success, a negative MCAMD_E* code otherwise; the message is
 *     available per host thread from mcamd_last_error(); nothing throws.
 *
 * Device data layouts
 *   activation ("padded NHWC"): fp16 [B][H+2][W+2][ld], a one-pixel zero halo on
 *     every side, `ld` channels per pixel (ld >= channels used, multiple of 8;
 *     a tensor may be a channel slice [choff, choff+C) of a wider buffer -- that
 *     is how route/concat is expressed).  The pointer passed is the address of
 *     padded pixel (b=0, hp=0, wp=0), channel 0.  The halo must be zero and is
 *     never written by the library.  Buffers must be preceded AND followed by a
 *     zeroed guard band of (round_up(W+3, 4) + 128) pixels (+ 64 elements): the 9-tap
 *     kernels read whole row windows around their pixel tiles, and the stem
 *     layer reads 32 contiguous halfs per pixel.
 *   raw conv output / gradient wrt a block output: fp16 [B*H*W][ld] (no halo).
 *   stem input (first layer, Cin = 3): padded NHWC with ld = 4 (channel 3 zero).
 *   activation, SHARED-HALO form (`pad` = 1 in the descriptors below; the engine uses it for its small images, W <= 26):
 *     the same tensor with ONE zero pixel between consecutive rows and ONE zero row between consecutive images --
 *     pixel (b, h, w) at ((b (H + 1) + h + 1) (W + 1) + w + 1) ld from a pointer that is the address of pixel
 *     (0, -1, -1); B (H + 1) (W + 1) + W + 2 pixels in all (the last image's bottom halo row and corner), guard bands as
 *     above.  The right halo of a row IS the left halo of the next one, the bottom halo row of an image the top one of the
 *     next: every 3x3 tap is still a constant shift, (ty - 1)(W + 1) + (tx - 1) pixels, and every kernel's addressing stays
 *     linear -- but the padded-pixel enumeration of the 9-tap weight gradient shrinks from (H + 2)(W + 2) to
 *     (H + 1)(W + 1) rows per image (13x13: 225 -> 196, -13 % of its MFMA work; conv19's weight gradient -19 %).
 *   packed weights: fp16 [Npad][K], see mcamd_pack_weights.
 *   master weights, masks, weight gradients: fp32 OIHW exactly as torch holds them.
 */
#ifndef MCAMD_H
#define MCAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCAMD_OK 0
#define MCAMD_EINVAL (-1)   /* bad argument / unsupported geometry */
#define MCAMD_ELAUNCH (-2)  /* HIP launch error */
#define MCAMD_EWORKSPACE (-3) /* workspace too small */

int mcamd_version(void);              /* 100*major + minor */
/* The MCAMD_* tuning switches are read from the environment once per process, at their first
 * use -- never per launch.  A process that changes one afterwards (tests, A/B runs) calls this to have them re-read. */
void mcamd_reload_config(void);
const char* mcamd_arch(void);         /* "gfx950" */
const char* mcamd_last_error(void);   /* per-thread, never NULL */

/* ------------------------------------------------------------------------- *
 * Convolution geometry: k x k cross-correlation, stride 1, zero pad (k-1)/2,
 * dilation 1, groups 1 -- the only form F.conv2d is called with on the hot
 * path (reference src/pruning/weightPruning/layers.py:60-64 via nets.py:796-806).
 * ------------------------------------------------------------------------- */
typedef struct mcamd_conv_geom {
    int32_t B, H, W;      /* batch, spatial size (output == input)            */
    int32_t ksize;        /* 1 or 3                                           */
    int32_t cin;          /* input channels of the weight tensor (any > 0).  The kernels consume
                             round_up(cin, 32) channels per pixel: the buffer slice must be that wide
                             and the extra channels must hold zeros.  3 when stem != 0. */
    int32_t cout;         /* output channels (any > 0)                        */
    int32_t x_ld;         /* channels per pixel of the input buffer           */
    int32_t x_choff;      /* first input channel inside the buffer            */
    int32_t stem;         /* 1: first-layer form, x is NHWC4 (x_ld == 4), cin == 3, ksize == 3 */
    int32_t pad;          /* 0: padded NHWC; 1: shared-halo form (above) of EVERY padded operand of the call -- x in
                             mcamd_conv_fwd, dy in mcamd_conv_dgrad, x and dy in mcamd_conv_wgrad.  stem == 0 only. */
    int32_t x_wrap;       /* mcamd_conv_fwd only, 0 = none.  Input channels >= x_wrap are read from channel - x_wrap of the
                             pixel: the split-operand forward on TWO activation planes [x_hi | x_lo], plane stride P,
                             with cin = 3 P, the K-concatenated weights [w_hi | w_hi | w_lo] (mcamd_pack_job.split) and
                             x_wrap = 2 P: the third part multiplies the hi plane again without a third copy of it.
                             P % 32 == 0; epilogue modes MCAMD_EPI_RAW_F32 / MCAMD_EPI_NCHW_F32; the buffer slice must hold
                             x_wrap channels. */
    int32_t x_f8;         /* mcamd_conv_fwd only, 0 = none.  P > 0 (P % 64 == 0, cin = 2 P, x_wrap = 0): the split-operand forward
                             with fp8 CORRECTION terms.  Channels [0, P) of the slice are the fp16 hi plane; the next P fp16
                             units hold 2 P OCP-e4m3 bytes [lo8 = e4m3(x_lo * 2^12) | x8 = e4m3(x * 2)] (mcamd_act_desc.planes 4),
                             the packed weights [w_hi | w8 = e4m3(w_hi * 2^e) | wlo8 = e4m3(w_lo * 2^(e + 11))], e = x_f8_wexp (mcamd_pack_job.split 2):
                             y = x_hi w_hi (fp16 MFMA) + 2^-(12 + e) (lo8 w8 + x8 wlo8) (block-scaled fp8 MFMA at twice the fp16
                             rate, same fp32 accumulators) -- x w to ~2^-15 instead of plain fp16's 2^-11, at 2/3 of the
                             x_wrap form's MFMA time and staged bytes.  x_choff = 0 (the e4m3 strings are addressed from the
                             pixel's first channel, also by a concat member writing at its offset).  Epilogue mode MCAMD_EPI_RAW_F32; only shapes for
                             which mcamd_conv_fwd_f8_ok() returns 1 (the ping-pong implicit-GEMM tiles).  Replaces the same
                             F.conv2d (reference src/pruning/weightPruning/layers.py:60-64). */
    int32_t x_f8_wexp;    /* with x_f8: the exponent the weight bytes were packed with, w8 = e4m3(w_hi * 2^x_f8_wexp), wlo8 =
                             e4m3(w_lo * 2^(x_f8_wexp + 11)) (mcamd_pack_job.f8_wexp; [-24, 40]).  Chosen per layer so that the
                             largest |w| lands in the upper binades of e4m3 (448): BatchNorm makes a layer's weight scale
                             arbitrary.  5 suits initialisation-sized weights (|w| <= 14). */
} mcamd_conv_geom;
int32_t mcamd_conv_fwd_f8_ok(const mcamd_conv_geom* g);   /* 1: mcamd_conv_fwd accepts this x_f8 geometry */

/* Output side of a convolution launch. */
#define MCAMD_EPI_RAW_F16 0   /* y: fp16 [M][y_ld] + optional per-channel partial sums (BN batch statistics) */
#define MCAMD_EPI_NCHW_F32 1  /* y: fp32 [B][cout][H][W] (+ bias)  -- the model's returned logits */
#define MCAMD_EPI_PAD_F16 2   /* y: padded NHWC fp16, leaky(acc*scale[c]+shift[c]) (inference, BN folded) */
#define MCAMD_EPI_RAW_F32 3   /* y: fp32 [M][y_ld], the accumulators unrounded (+ optional partial sums taken from the
                                 fp32 values) -- the "fp16x3" precision mode, see mcamd_act_desc.planes */
typedef struct mcamd_conv_epilogue {
    int32_t mode;
    int32_t y_ld, y_choff;     /* modes 0, 2 and 3 */
    void* y;
    const float* bias;         /* mode 1, may be NULL */
    float* stats;              /* modes 0 and 3, may be NULL: fp32 [stats_rows][2][stats_ld]; row p holds the
                                  per-channel sums (index 0) and sums of squares (index 1) over the pixels
                                  that persistent workgroup p processed (fixed order: deterministic) */
    int32_t stats_rows;        /* must equal mcamd_conv_stats_rows_mode(geom, mode) */
    int32_t stats_ld;          /* >= round_up(cout, 256) */
    const float* scale;        /* mode 2, may be NULL (=1) */
    const float* shift;        /* mode 2, may be NULL (=0) */
    float slope;               /* mode 2: negative-side slope (0.1 leaky, 1.0 linear) */
    int32_t* overflow;         /* modes 0 and 2, may be NULL: device flag, set to 1 when a value had to be clamped to
                                  the fp16 range (+-65504) on its way out.  fp16 outputs saturate instead of becoming
                                  inf; the scaled gradients of the backward pass (grad_scale x dX) are where that can
                                  happen, and the caller decides (train.py skips the step and halves grad_scale). */
    int32_t dst_mode;          /* mode 2 only: MCAMD_DST_PLAIN (0), MCAMD_DST_POOL or MCAMD_DST_REORG -- the inference
                                  epilogue fused with the MaxPool(2,2) / Reorg(2) that follows the block (nets.py:821,
                                  648-667): `y` is then the padded NHWC buffer at the POOLED resolution (H/2 x W/2; reorg:
                                  4 x cout channels from y_choff), H and W must be even, and the forward launch enumerates
                                  its output pixels window by window.  Forward only. */
    void* y2;                  /* dst_mode POOL, may be NULL: a second, FULL-resolution padded copy of leaky(bn(conv)) (the
                                  route that reads the block beside its pool: conv13 of yolov2-voc.cfg) */
    int32_t y2_ld, y2_choff;
    /* (mode 2 writes the standard padded form: inference engines do not use the shared-halo one) */
    int32_t concurrent;        /* mcamd_conv_dgrad only, 0 / 1: the caller runs other kernels on another stream at the
                                  same time (the training engine: the weight gradients of the layers behind).  The launch
                                  then picks the workgroup tile with the least CU-time even if it fills only 40-80 % of the
                                  CUs, instead of the tile with the shortest launch on an otherwise idle GPU. */
} mcamd_conv_epilogue;

/* Rows of the BatchNorm partial-sum slab a forward launch of this geometry writes (epilogue mode 0). */
int32_t mcamd_conv_stats_rows(const mcamd_conv_geom* g);
/* The same for a given epilogue mode (MCAMD_EPI_RAW_F16 or MCAMD_EPI_RAW_F32): the rows of the kernel mcamd_conv_fwd
 * launches for (geometry, mode).  The queries below and the launch ask one route function, so a slab sized here is the
 * slab the launch accepts. */
int32_t mcamd_conv_stats_rows_mode(const mcamd_conv_geom* g, int32_t mode);

/* Workgroup tile {BM, BN, BK, kernel} the forward (dgrad == 0) or dgrad launch (1; 2 = with epilogue.concurrent set) of
 * this geometry uses, from the same route function as the launch.  Forward: a training launch (with a statistics slab),
 * epilogue mode 3 for x_wrap / x_f8 geometries (they exist with the fp32 epilogues only), else mode 0; dgrad: mode 0.
 * kernel 0 = igemm_kernel<BM,BN,..,BK,..> (one tap per K chunk),
 * 2 = igemm_pp_kernel (ping-pong, one workgroup per CU), 1 = stem_fwd_kernel (first layer, no LDS staging),
 * 4 = small3x3_kernel (narrow 3x3 layers on huge images, no LDS staging), 5 = win3x3_kernel (rolling LDS window),
 * 6 = wres_kernel (3x3 layers with one 64-channel input block: weights resident in registers, one activation window per
 * M tile of 128 padded pixels), 7 = small3x3_split_kernel (the 32 -> <= 64 channel 3x3 layer on split operands at
 * x_choff 0, fp32 output; BN = round_up(cout, 32), BK = the 96 K-concatenated channels). */
int mcamd_conv_tile_info(const mcamd_conv_geom* g, int32_t dgrad, int32_t out[4]);
/* The same route function's whole answer {BM, BN, BK, kernel, rows} for any launch: dir 0 = mcamd_conv_fwd, 1 = mcamd_conv_dgrad,
 * 2 = mcamd_conv_dgrad with epilogue.concurrent set; `mode` / `dst_mode` = the epilogue's; stats != 0: the epilogue has a
 * statistics slab.  rows = the persistent workgroups along M (the rows of that slab; 0 for win3x3_kernel).  Host logic
 * only: no device is touched.  It answers for the combination given, whether or not the launch entry accepts it. */
int mcamd_conv_route_info(const mcamd_conv_geom* g, int32_t dir, int32_t mode, int32_t dst_mode, int32_t stats, int32_t out[5]);

/* Packed-weight sizes (elements of fp16) for a geometry. */
int64_t mcamd_packed_elems_fwd(const mcamd_conv_geom* g);
int64_t mcamd_packed_elems_dgrad(const mcamd_conv_geom* g);

/* Physical channel order of one convolution (NULL pointers = identity).  With filter pruning the engine keeps
 * the surviving filters first and computes only those: `g->cout` / `g->cin` then describe the PHYSICAL problem
 * and the weight / mask / gradient tensors keep the module's OIHW order with `g->cin` input channels per filter:
 * physical filter n is tensor row rows[n], physical input channel c is tensor column cols[c]. */
typedef struct mcamd_chan_map {
    const int32_t* rows;   /* device int32[g->cout] or NULL */
    const int32_t* cols;   /* device int32[g->cin] or NULL */
} mcamd_chan_map;

/* OIHW fp32 master (optionally * mask) -> fp16 kernel layouts.  Replaces the per-forward
 * `self.weight * mask_var` of layers.py:59 (done once per optimizer step here).
 *   fwd  : [Npad][kpos(t, c)] = w[n][c][ty][tx],  t = ty*k + tx;  Npad = roundup(cout,256); pad rows zero
 *          (stem: [Npad][ty*32 + tx*4 + c], other slots zero)
 *   dgrad: [Cpad][kpos(t, n)] = w[n][c][k-1-ty][k-1-tx]; cout_p = roundup(cout,32); Cpad = roundup(cin,256)
 *   kpos(t, c) = (c / kb) * k*k*kb + t * kb + c % kb over the padded channel count chp (cin_tap = roundup(cin,32)
 *   or cout_p), kb = 64 if chp % 64 == 0 else 32: the K axis runs [channel block][tap][channel in block], so the
 *   k*k shifted reads of one activation line are consecutive K chunks (L2 hits instead of k*k streams).
 * Either destination may be NULL.  `map` (may be NULL): gather rows / columns of w and mask, see mcamd_chan_map. */
int mcamd_pack_weights(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw,
                       const mcamd_chan_map* map, void* wp_fwd, void* wp_dgrad, void* stream);

/* All layers of a network in ONE launch (the per-step re-pack of engine.py): `jobs_dev` is a DEVICE array of
 * `njobs` descriptors, one per layer.  A workgroup takes a 32-filter x 32-channel tile of one layer: the
 * k*k taps of every (filter, channel) pair are read as one contiguous run (x mask), transposed through LDS
 * and written to BOTH packed layouts in 64-byte pieces, so the fp32 master and the mask are read once.
 * Only real entries are written -- pad rows / pad channels of the destinations must already be zero
 * (they never change).  The stem layer is not supported here (use mcamd_pack_weights). */
typedef struct mcamd_pack_job {
    const float* w;            /* OIHW fp32 master */
    const float* mask;         /* OIHW fp32 or NULL */
    void* dst_fwd;             /* fp16 forward layout, or NULL */
    void* dst_dgrad;           /* fp16 dgrad layout, or NULL */
    const int32_t* rows;       /* channel maps as in mcamd_chan_map, or NULL */
    const int32_t* cols;
    int64_t first_tile;        /* sum of ceil(cout/32)*ceil(cin/32) over the preceding jobs */
    int32_t cout, cin, ksize;  /* physical geometry */
    int32_t split;             /* 0: plain fp16 forward packing.  1: the split-operand forward packing of the "fp16x3" /
                                  "mixed" precisions, [w_hi | w_hi | w_lo] along the input channels of a 3 * cin wide row
                                  (w_hi = fp16(w * mask), w_lo = fp16(w * mask - w_hi)), to be multiplied with
                                  [x_hi | x_lo | x_hi] activation planes; dst_fwd then has the size of a geometry with
                                  3 * cin input channels.  2: the fp8-correction packing of mcamd_conv_geom.x_f8,
                                  [w_hi fp16 | w8 | wlo8 e4m3 bytes] in a row of 2 * cin fp16 units per tap (cin % 64 == 0).
                                  The dgrad packing is plain in every case. */
    int32_t f8_wexp;           /* split 2: w8 = e4m3(w_hi * 2^f8_wexp), wlo8 = e4m3(w_lo * 2^(f8_wexp + 11)); the consumer's
                                  mcamd_conv_geom.x_f8_wexp must say the same */
} mcamd_pack_job;
int mcamd_pack_weights_many(const mcamd_pack_job* jobs_dev, int32_t njobs, int64_t total_tiles, void* stream);

/* y = conv(x, w) -- replaces F.conv2d at layers.py:60-64. */
int mcamd_conv_fwd(const mcamd_conv_geom* g, const void* x, const void* wp_fwd,
                   const mcamd_conv_epilogue* epi, void* stream);

/* ------------------------------------------------------------------------- *
 * 2:4 structured sparsity (an addition beyond the reference): inference forward on v_smfmac_f32_32x32x32_f16 for
 * layers whose mask keeps at most 2 of every 4 consecutive input channels at each (filter, tap) -- nm_prune.
 * ------------------------------------------------------------------------- */
/* 1: mcamd_conv_fwd_sparse24 / mcamd_pack_sparse24 accept this geometry (stem == 0, ksize 1 or 3, cin % 4 == 0,
 * cout % 8 == 0, x_wrap == 0, x_f8 == 0, the input slice of round_up(cin, 32) channels inside x_ld). */
int32_t mcamd_conv_fwd_sparse24_ok(const mcamd_conv_geom* g);
/* Sizes of the packed 2:4 operands: out[0] = fp16 kept values, out[1] = 16-bit index words. */
int mcamd_sparse24_elems(const mcamd_conv_geom* g, int64_t out[2]);
/* The kernel instance mcamd_conv_fwd_sparse24 launches for this geometry, from the launch's own choice (host logic only, no
 * GPU): out = {bmw, bnp, bk, stages, mtiles, ntiles, grid} -- a workgroup tile of bmw filters x bnp pixels, K chunks of bk
 * (the channel block of the packed K order), LDS ring stages, the tiles along the pixels and the filters, and the blocks
 * launched (whole rounds of 8 pixel tiles).  MCAMD_SPARSE_WIDE=0 removes the 256-filter tile. */
int mcamd_conv_fwd_sparse24_info(const mcamd_conv_geom* g, int32_t out[7]);
/* OIHW fp32 master (* mask, may be NULL) -> the 2:4 packing the sparse forward stages:
 *   wsp: fp16 [Npad][ktot / 2], Npad = round_up(cout, 256), ktot = k*k * round_up(cin, 32): the dense forward row
 *        (K order of mcamd_pack_weights) with each group of 4 consecutive k reduced to its 2 kept values, in k order;
 *   idx: uint16 [ktot / 32][Npad][2]: word h of K32 chunk q of row n holds, for the 8 kept values of k [32 q + 16 h, +16),
 *        the offset of kept value j inside its group of 4 at bits [2 j, 2 j + 2).
 * The kept entries of a group are its non-zeros of w * mask (the first two when the mask does not conform); a group with
 * fewer gets distinct indices with zero values.  Every row up to Npad is written. */
int mcamd_pack_sparse24(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wsp, void* idx, void* stream);
/* y = leaky(conv(x, w) * scale + shift) from the 2:4 packing: epilogue mode MCAMD_EPI_PAD_F16 only (with dst_mode PLAIN /
 * POOL / REORG and y2 exactly as mcamd_conv_fwd), for geometries mcamd_conv_fwd_sparse24_ok() accepts, both `pad` forms of
 * x.  The result equals mcamd_conv_fwd's on the same masked weights up to fp32 summation order. */
int mcamd_conv_fwd_sparse24(const mcamd_conv_geom* g, const void* x, const void* wsp, const void* idx,
                            const mcamd_conv_epilogue* epi, void* stream);

/* ------------------------------------------------------------------------- *
 * Block-sparse fp16 inference forward (an addition beyond the reference; conv_bsparse.hip, Darknet.sparse = "block").
 * The packed K axis of mcamd_pack_weights runs [channel block][tap][kb channels], so K chunk q of kb columns is one
 * (channel block, tap) pair.  For every N tile of 64 filters a list names the chunks the tile multiplies, in ascending
 * q; a chunk whose 64 x kb weights are all zero adds exactly +0 to every accumulator, so a launch on the lists of
 * mcamd_bsparse_lists equals the same launch on full lists bit for bit, and that one walks mcamd_conv_fwd's igemm MFMA
 * sequence.  The weights are the dense packing of mcamd_pack_weights: no second format.
 * ------------------------------------------------------------------------- */
/* 1: the entries below accept this geometry (stem == 0, ksize 1 or 3, cin % 32 == 0 -- cin_tap == cin --, cout % 8 == 0,
 * x_wrap == 0, x_f8 == 0, the input slice inside x_ld). */
int32_t mcamd_conv_fwd_bsparse_ok(const mcamd_conv_geom* g);
/* Sizes of the lists (int32 entries): out[0] = ntiles = ceil(cout / 64) counts, out[1] = ntiles * nchunks list entries,
 * nchunks = k*k * cin / kb. */
int mcamd_bsparse_elems(const mcamd_conv_geom* g, int64_t out[2]);
/* count[nt] and list[nt][0 .. count[nt]) from the packed forward weights: the chunks q with any non-zero fp16 value
 * (-0 counts as zero) in rows [64 nt, 64 nt + 64), columns [q kb, q kb + kb), ascending.  One wave ballot per (tile,
 * chunk) and a scan in q order: no atomics, no host synchronisation.  Entries behind the count are written as 0. */
int mcamd_bsparse_lists(const mcamd_conv_geom* g, const void* wp_fwd, int32_t* count, int32_t* list, void* stream);
/* y = leaky(conv(x, w) * scale + shift) over the listed chunks: epilogue mode MCAMD_EPI_PAD_F16 only (dst_mode PLAIN /
 * POOL / REORG, y2, channel offsets and the overflow flag exactly as mcamd_conv_fwd), both `pad` forms of x.  A count
 * outside [0, nchunks] or an index outside [0, nchunks) is clamped into its range. */
int mcamd_conv_fwd_bsparse(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const int32_t* count,
                           const int32_t* list, const mcamd_conv_epilogue* epi, void* stream);
/* The kernel instance mcamd_conv_fwd_bsparse launches for this geometry, from the launch's own choice (host logic only, no
 * GPU): out = {bm, bn, bk, stages, mtiles, ntiles, grid} -- a workgroup tile of bm pixels (MCAMD_BSPARSE_BM: 64, else 128) x
 * bn = 64 filters, K chunks of bk = kb, LDS ring stages, the tiles along the pixels and the filters, and the blocks launched
 * (whole rounds of 8 pixel tiles). */
int mcamd_conv_fwd_bsparse_info(const mcamd_conv_geom* g, int32_t out[7]);

/* ------------------------------------------------------------------------- *
 * The training form of the block-sparse kernel (Darknet.sparse_train = "block"): the same K loop over the
 * listed chunks with the raw fp16 epilogue (MCAMD_EPI_RAW_F16), for the forward GEMM and for the dgrad GEMM.  The dgrad
 * packing of mcamd_pack_weights is [Cpad][k*k * cout_p] with the forward's K order [channel block][tap][kb] over cout_p
 * (kb_d = 64 when cout_p % 64 == 0, else 32), so a K chunk of a 64-row N tile (64 input channels) is one (cout block,
 * flipped tap) pair: when cout_p % 64 == 0, exactly one block of block_prune's masks, seen from the other side.  The
 * lists are read from the packed values, so any mask is correct.  `dgrad` below: 0 the forward launch, 1 the dgrad launch.
 * ------------------------------------------------------------------------- */
/* 1: the launch of that direction accepts the geometry.  Forward: as mcamd_conv_fwd_bsparse_ok.  dgrad: stem == 0, x_wrap ==
 * 0, x_f8 == 0, ksize 1 or 3, cin % 8 == 0 (the launch also wants the slice of dy inside dy_ld).  Host logic only. */
int32_t mcamd_conv_bsparse_train_ok(const mcamd_conv_geom* g, int32_t dgrad);
/* The instance the launch of that direction takes, from its own choice (host logic only): out as
 * mcamd_conv_fwd_bsparse_info's {bm, bn, bk, stages, mtiles, ntiles, grid}; dgrad: ntiles over cin, bk = kb_d. */
int mcamd_conv_bsparse_train_info(const mcamd_conv_geom* g, int32_t dgrad, int32_t out[7]);
/* Rows of the statistics slab of mcamd_conv_fwd_bsparse_raw: one per pixel tile (= mtiles; the grid is not persistent).
 * 0: the geometry is refused. */
int32_t mcamd_conv_bsparse_raw_stats_rows(const mcamd_conv_geom* g, int32_t dgrad);
/* mcamd_bsparse_elems / mcamd_bsparse_lists on the dgrad packing: ntiles = ceil(cin / 64), nchunks = k*k * cout_p / kb_d. */
int mcamd_bsparse_elems_dgrad(const mcamd_conv_geom* g, int64_t out[2]);
int mcamd_bsparse_lists_dgrad(const mcamd_conv_geom* g, const void* wp_dgrad, int32_t* count, int32_t* list, void* stream);
/* y[M][y_ld] (at y_choff) = conv(x, w) over the listed chunks, fp16 saturated at +-65504 (never inf; epi->overflow is set
 * where a value was clamped).  epi->mode must be MCAMD_EPI_RAW_F16 (else MCAMD_EINVAL); both `pad` forms of x.  With
 * epi->stats: per channel the sum and the sum of squares of the values AS STORED (mcamd_conv_fwd's convention for this
 * mode), one slab row [2][stats_ld] per pixel tile, stats_rows = mcamd_conv_bsparse_raw_stats_rows(g, 0).  A tile whose
 * count is 0 stores zeros and zero sums; foreign counts and indices are clamped as in mcamd_conv_fwd_bsparse. */
int mcamd_conv_fwd_bsparse_raw(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const int32_t* count,
                               const int32_t* list, const mcamd_conv_epilogue* epi, void* stream);
/* gin[M][y_ld] (at y_choff) = mcamd_conv_dgrad's result over the listed chunks of mcamd_bsparse_lists_dgrad: the same
 * operands and geometry set-up; MCAMD_EPI_RAW_F16 without statistics only, with the overflow flag.  epi->concurrent is
 * accepted and ignored (one tile shape). */
int mcamd_conv_dgrad_bsparse(const mcamd_conv_geom* g, const void* dy, int32_t dy_ld, int32_t dy_choff, const void* wp_dgrad,
                             const int32_t* count, const int32_t* list, const mcamd_conv_epilogue* epi, void* stream);

/* ------------------------------------------------------------------------- *
 * Split-K forward for low-batch fp16 inference (an addition beyond the reference; conv_splitk.hip, Darknet.splitk).
 * A layer of few output pixels gives mcamd_conv_fwd a handful of workgroups that each walk the whole K axis; here
 * workgroup (tile, slice s) of a first launch multiplies the K chunks [floor(s n / S), floor((s + 1) n / S)) of the
 * tile's n = ktot / bk chunks and stores its unrounded fp32 accumulators to slab s of `workspace`; a second launch on
 * the same stream sums the S slabs of every element in slice order in fp32 and applies mcamd_conv_fwd's epilogue.  The
 * result is a function of the operands and S only (no atomics, no workgroup waits for another); with S = 1 it is
 * mcamd_conv_fwd's igemm result bit for bit.
 *
 * Geometries: stem == 0, pad == 0, x_wrap == 0, x_f8 == 0, ksize 1 or 3.  Epilogues: MCAMD_EPI_PAD_F16 (dst_mode
 * PLAIN / POOL (+ y2) / REORG) and MCAMD_EPI_RAW_F16 with stats == NULL.  Same packed weights as mcamd_conv_fwd.
 * ------------------------------------------------------------------------- */
typedef struct mcamd_splitk_info {
    int32_t slices;          /* 1 = the policy does not split this launch */
    int32_t bm, bn, bk;      /* workgroup tile of the partial kernel */
    int32_t chunks;          /* ktot / bk */
    int32_t tiles;           /* M tiles x N tiles */
    int64_t workspace_bytes; /* what mcamd_conv_fwd_splitk needs for `slices` */
    int32_t stages;          /* LDS ring depth of the partial kernel instance */
    int32_t mtiles, ntiles;  /* partial tiles along the pixels and the filters (tiles = mtiles x ntiles) */
    int32_t finish_rows, finish_cols; /* the finish kernel's tile: pixels x channels */
} mcamd_splitk_info;
/* Host logic only.  slices = 0 asks the policy (the largest S <= MCAMD_SPLITK_CUS / tiles that leaves every slice at
 * least MCAMD_SPLITK_MIN_CHUNKS chunks, clamped to [1, 16]); slices > 0 sizes a forced count in [1, chunks]. */
int mcamd_conv_fwd_splitk_info(const mcamd_conv_geom* g, int32_t mode, int32_t dst_mode, int32_t slices,
                               mcamd_splitk_info* out);
/* The two launches.  slices as above; workspace: at least the workspace_bytes the query returns for the same
 * arguments, 16-byte aligned, free again once the call's launches have run. */
int mcamd_conv_fwd_splitk(const mcamd_conv_geom* g, const void* x, const void* wp_fwd, const mcamd_conv_epilogue* epi,
                          int32_t slices, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * fp8 (OCP e4m3) quantised inference (an addition beyond the reference; conv_q8.hip, Darknet.precision = "fp8").
 *   q(v) = round-to-nearest-even to e4m3 of v clamped to [-448, 448].
 *   activations: bytes q(2 x) in a padded NHWC BYTE buffer [B][H+2][W+2][ld] (or the shared-halo form), halo bytes 0x00;
 *   weights, per filter f: a = max |w * mask|, (m, x) = frexp(a), e_f = 9 - x if m <= 0.875 else 8 - x (0 for an all-zero
 *   filter), bytes q(w * mask * 2^e_f): the filter's largest weight lands in (224, 448];
 *   output: v = leaky(scale_f * 2^-(e_f + 1) * S + shift_f), S = the fp32-accumulated sum of byte products.
 *   S is an fp32 sum of the exact products (fp16 MFMAs on the bytes converted in registers).  MCAMD_Q8_MFMA=1 multiplies the
 *   bytes on the block-scaled fp8 MFMA instead: 1.41x instead of 1.01x the fp16 forward of YOLOv2-VOC at B = 128, but that instruction truncates
 *   inside groups of 8 products and a few 1e-4 of the output bytes come out one code off.
 * ------------------------------------------------------------------------- */
/* 1: mcamd_conv_fwd_q8 / mcamd_pack_q8 accept this geometry: stem == 0, ksize 1 or 3, cin % 64 == 0, cout % 8 == 0,
 * x_wrap == 0, x_f8 == 0, x_ld % 16 == 0, x_choff % 16 == 0, the slice of cin channels inside x_ld.  Any batch size. */
int32_t mcamd_conv_fwd_q8_ok(const mcamd_conv_geom* g);
/* Sizes of the packed operands: out[0] = weight bytes (Npad * k*k * cin, Npad = round_up(cout, 256)), out[1] = int32
 * exponents (Npad). */
int mcamd_q8_elems(const mcamd_conv_geom* g, int64_t out[2]);
/* OIHW fp32 master (* mask, may be NULL) -> wq: bytes [Npad][kpos], kpos(t, c) = (c / 64) * k*k*64 + t * 64 + c % 64;
 * wexp: int32 [Npad] (e_f; pad rows: zero bytes, exponent 0).  Exponents are computed on the device. */
int mcamd_pack_q8(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wq, int32_t* wexp, void* stream);
/* The quantised block: epilogue mode MCAMD_EPI_PAD_F16 (inference; MCAMD_EPI_RAW_F32: the training form below), dst_mode PLAIN / POOL / REORG and y2 as mcamd_conv_fwd.
 * y_f8 / y2_f8 != 0: that destination is a padded NHWC BYTE buffer and receives q(2 v) (y_ld / y_choff count bytes);
 * 0: fp16 as mcamd_conv_fwd writes it.  Both `pad` forms of x. */
int mcamd_conv_fwd_q8(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                      const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, void* stream);
/* The kernel instance an fp8 block launches for this geometry, from the launches' own choice (host logic only, no GPU).
 * form: 0 mcamd_conv_fwd_q8 with the inference epilogue, 1 mcamd_conv_fwd_q8 with MCAMD_EPI_RAW_F32, 2 mcamd_conv_fwd_q8_slim
 * with a border table (without one it launches form 0's kernel on the same tile; the geometry is held to
 * mcamd_conv_fwd_q8_slim_ok), 3 mcamd_conv_fwd_q8_sparse24.  out = {bmw, bnp, f8mfma, stages, mtiles, ntiles, grid} -- a
 * workgroup tile of bmw filters x bnp pixels, whether MCAMD_Q8_MFMA selects the fp8 MFMA, LDS ring stages, the tiles along
 * the pixels and the filters, and the blocks launched (whole rounds of 8 pixel tiles). */
int mcamd_conv_fwd_q8_info(const mcamd_conv_geom* g, int32_t form, int32_t out[7]);
/* The cast pass of an fp16 -> fp8 edge: fp16 [pixels][src_ld] channels [src_choff, +C) -> bytes q(2 x) [pixels][dst_ld]
 * channels [dst_choff, +C); C, the leading dimensions and offsets multiples of 8.  Halo pixels are pixels like any other. */
int mcamd_cast_q8(const void* src, int64_t pixels, int32_t src_ld, int32_t src_choff, int32_t C, void* dst, int32_t dst_ld,
                  int32_t dst_choff, void* stream);

/* ---------------------------------------------------------------------------
 * Split-K form of the quantised block for low-batch inference (an addition beyond the reference; conv_q8_splitk.hip,
 * Darknet.precision = "fp8-splitk"): mcamd_conv_fwd_splitk's launch design on mcamd_conv_fwd_q8's operands.
 * Workgroup (tile of 64 filters x 64 pixels, slice s) of a first launch multiplies the 64-byte K chunks
 * [floor(s n / S), floor((s + 1) n / S)) of the tile's n = k*k * cin / 64 chunks -- in the MFMA form MCAMD_Q8_MFMA selects --
 * and stores its unrounded fp32 accumulators to slab s of `workspace` ([S][Mpad][Npad] fp32, whole tiles); a second launch on
 * the same stream sums the S slabs of every element in slice order in fp32 and applies mcamd_conv_fwd_q8's epilogue,
 * v = leaky(scale_f * 2^-(e_f + 1) * S + shift_f), written as q(2 v) bytes or saturated fp16 per destination.  No atomics,
 * no workgroup waits for another: the result is a function of the operands, the MFMA form and S only; with S = 1 it is
 * mcamd_conv_fwd_q8's result code for code, and it differs from it by the order of the fp32 sum only for any S.
 *
 * Geometries: mcamd_conv_fwd_q8_ok and pad == 0.  Epilogue: MCAMD_EPI_PAD_F16 (dst_mode PLAIN / POOL (+ y2) / REORG) with
 * stats == NULL.  Operands: exactly mcamd_conv_fwd_q8's (mcamd_pack_q8's bytes and exponents, the same byte buffer).
 * ------------------------------------------------------------------------- */
/* Host logic only.  The policy is mcamd_conv_fwd_splitk_info's (MCAMD_SPLITK_CUS, MCAMD_SPLITK_MIN_CHUNKS, the clamp to 16)
 * on chunks of 64 k: slices = 0 asks it, slices > 0 sizes a forced count in [1, chunks].  out->bm = pixels, bn = filters,
 * bk = 64 of the partial kernel's tile. */
int mcamd_conv_fwd_q8_splitk_info(const mcamd_conv_geom* g, int32_t dst_mode, int32_t slices, mcamd_splitk_info* out);
/* The two launches.  y_f8 / y2_f8 as mcamd_conv_fwd_q8; slices as above; workspace: at least the workspace_bytes the query
 * returns for the same arguments, 16-byte aligned, free again once the call's launches have run.  Everything refused is
 * refused before the first launch. */
int mcamd_conv_fwd_q8_splitk(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                             const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, int32_t slices, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Block-sparse form of the quantised block (an addition beyond the reference; conv_q8_bsparse.hip, Darknet.precision =
 * "fp8-block"): mcamd_conv_fwd_q8 on its 64-filter x 128-pixel tile, taking the 64-byte K chunks of each N
 * tile from a list as mcamd_conv_fwd_bsparse does.  The fp8 K order [channel block of 64][tap][64 channels] makes chunk q one
 * (channel block, tap) pair of 64 filters: one block of block_prune's masks (cin % 64 == 0, so kb = 64).
 *   lists     count: int32 [ntiles], ntiles = ceil(cout / 64); list: int32 [ntiles][nchunks], nchunks = k*k * cin / 64.
 *             Entries [0, count[nt]) of row nt are the chunks tile nt multiplies, ascending.
 *   operands  exactly mcamd_conv_fwd_q8's: mcamd_pack_q8's bytes [Npad][k*k * cin] and exponents, the same byte buffer.
 * A chunk whose 64 x 64 weight bytes are all zero codes (0x00 or 0x80) adds +-0 to accumulators that start at +0: in the
 * default MFMA form a launch on mcamd_q8_bsparse_lists' lists equals the same launch on full lists bit for bit, and that one
 * feeds every accumulator mcamd_conv_fwd_q8's instruction sequence, so it equals that entry bit for bit.  The same holds
 * on the fp8 MFMA (MCAMD_Q8_MFMA=1), by measurement: all-zero A bytes leave C as it is (the tests assert it).
 * ------------------------------------------------------------------------- */
/* 1: the entries below accept this geometry: what mcamd_conv_fwd_q8_ok accepts, with cin % 64 == 0 and pad == 0. */
int32_t mcamd_conv_fwd_q8_bsparse_ok(const mcamd_conv_geom* g);
/* Sizes of the lists (int32 entries): out[0] = ntiles = ceil(cout / 64) counts, out[1] = ntiles * nchunks list entries,
 * nchunks = k*k * cin / 64. */
int mcamd_q8_bsparse_elems(const mcamd_conv_geom* g, int64_t out[2]);
/* count[nt] and list[nt][0 .. count[nt]) from mcamd_pack_q8's bytes wq [Npad][k*k * cin]: the chunks q with any byte b,
 * b & 0x7f != 0 (both e4m3 zeros are zeros), in rows [64 nt, 64 nt + 64), columns [64 q, 64 q + 64), ascending.  One wave
 * ballot per (tile, chunk) and a scan in q order: no atomics, no host synchronisation.  Entries behind the count are written
 * as 0.  Refused above 8192 chunks.  From the bytes, not the mask: a kept weight that rounds to a zero byte is skipped too. */
int mcamd_q8_bsparse_lists(const mcamd_conv_geom* g, const void* wq, int32_t* count, int32_t* list, void* stream);
/* mcamd_conv_fwd_q8 over the listed chunks: epilogue mode MCAMD_EPI_PAD_F16 only; dst_mode PLAIN / POOL / REORG, y2, y_f8 /
 * y2_f8 and the overflow flag as there.  A count outside [0, nchunks] or an index outside [0, nchunks) is clamped into its
 * range.  count == 0: the tile's outputs are leaky(shift_f). */
int mcamd_conv_fwd_q8_bsparse(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp, const int32_t* count,
                              const int32_t* list, const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, void* stream);
/* The kernel instance mcamd_conv_fwd_q8_bsparse launches for this geometry (host logic only, no GPU): out as
 * mcamd_conv_fwd_q8_info's -- always the 64 x 128 tile with a 3-stage ring, in the MFMA form MCAMD_Q8_MFMA selects. */
int mcamd_conv_fwd_q8_bsparse_info(const mcamd_conv_geom* g, int32_t out[7]);

/* ---------------------------------------------------------------------------
 * fp8 inference of slim_export models (an addition beyond the reference): the fp8 block above for an input
 * channel count that is a multiple of 8 only, and with the border table of a conv that lost input channels (slim.py) in
 * the epilogue.  With cin_pad = round_up(cin, 64):
 *   weights   rows of cin_pad channels per tap, kpos(t, c) as above over cin_pad channels; the bytes of the channels
 *             [cin, cin_pad) are 0x00; e_f from max |w * mask| over the real channels;
 *   K loop    the one of mcamd_conv_fwd_q8 over cin_pad channels: the bytes it reads behind the slice, channels [x_choff +
 *             cin, x_choff + cin_pad) of the same pixel, must lie inside x_ld; they may hold anything a byte buffer holds
 *             (never-written 0x00, or another tensor's codes: q() never stores a NaN code) -- every such product is an
 *             exact 0, so the result is bit-identical to mcamd_conv_fwd_q8 on the weights zero-extended to cin_pad channels;
 *   output    v = leaky(scale_f * (2^-(e_f + 1) * S + border[cls(h, w)][f]) + shift_f), evaluated in fp32; cls has bit 0
 *             for h == 0, bit 1 for h == H - 1, bit 2 for w == 0, bit 3 for w == W - 1 (mcamd_act_desc.border); the entries
 *             are used as given (fp32, not quantised); border == NULL: no term.
 * ------------------------------------------------------------------------- */
/* mcamd_conv_fwd_q8_ok's predicate with cin % 8 == 0 in place of cin % 64 == 0 and x_choff + round_up(cin, 64) <= x_ld in
 * place of x_choff + cin <= x_ld.  Needs no device. */
int32_t mcamd_conv_fwd_q8_slim_ok(const mcamd_conv_geom* g);
/* out[0] = weight bytes (Npad * k*k * round_up(cin, 64), Npad = round_up(cout, 256)), out[1] = int32 exponents (Npad). */
int mcamd_q8_slim_elems(const mcamd_conv_geom* g, int64_t out[2]);
/* mcamd_pack_q8 into rows of round_up(cin, 64) channels per tap (pad channels 0x00; every row up to Npad is written). */
int mcamd_pack_q8_slim(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wq, int32_t* wexp,
                       void* stream);
/* The block: epi->mode MCAMD_EPI_PAD_F16 only; dst_mode, y2, y_f8 / y2_f8 as mcamd_conv_fwd_q8.  border: fp32 [16][border_ld]
 * or NULL; border_ld >= cout, border_ld % 4 == 0.  Both MCAMD_Q8_MFMA forms, both `pad` forms of x, any batch size. */
int mcamd_conv_fwd_q8_slim(const mcamd_conv_geom* g, const void* x8, const void* wq, const int32_t* wexp,
                           const mcamd_conv_epilogue* epi, const float* border, int32_t border_ld, int32_t y_f8, int32_t y2_f8,
                           void* stream);

/* ---------------------------------------------------------------------------
 * fp8 quantisation-aware training (an addition beyond the reference; Darknet.precision = "fp8-qat"): the
 * training-mode forward of an fp8 block runs in the deployment arithmetic above, its backward is straight-through.
 *   forward   a8 = q(2 x) input codes, (w8, e_f) re-quantised from w = weight * mask every step (mcamd_pack_q8);
 *             raw output y[m][f] = 2^-(e_f + 1) * sum a8 * w8, fp32 [B*H*W][y_ld] -- the convolution of x_q = deq(a8) / 2
 *             with w_q = deq(w8) * 2^-e_f (the power of two is exact);
 *             BatchNorm takes batch statistics of those fp32 values (biased variance; running statistics updated as
 *             nn.BatchNorm2d does: mcamd_bn_coeffs on the slab below); v = leaky(scale_f * y + shift_f);
 *             a destination the engine holds as bytes receives q(2 v) (POOL: q of 2 x the window maximum; REORG and the
 *             full-resolution copy mapped as in inference), ONE rounding from fp32, and the fp16 buffer of the same tensor
 *             deq(that byte) / 2, exact in fp16 (mcamd_act_desc.dst_q8 / dst2_q8); a destination a non-fp8 block reads
 *             receives fp16(v);
 *             at an fp16 -> fp8 edge the consumer's codes are q(2 x16) and mcamd_cast_q8_train writes deq(code) / 2 back
 *             over the fp16 slice: the values the consumer's weight gradient multiplies.
 *   backward  both quantisers are the identity (straight-through), WITHOUT a clipping mask: after BatchNorm |2 v| > 448
 *             does not occur in practice.  G -> pool / reorg / route, LeakyReLU and BatchNorm backward from the saved fp32 y
 *             (mcamd_bn_act_bwd, y_dtype 1: the pooled argmax is the forward's, taken on the unrounded activations) -> dY;
 *             dX = dgrad(dY, fp16(w_q)), dW = wgrad(dY, x_q) * mask; master weights fp32.  fp16(w_q) is exact for
 *             initialisation-sized weights (e4m3 has 4 significant bits; w_q leaves fp16's normal range only below 2^-14).
 *   An inference-mode forward under "fp8-qat" is the "fp8" engine's, bit for bit.
 * ------------------------------------------------------------------------- */
/* mcamd_conv_fwd_q8 also takes epilogue mode MCAMD_EPI_RAW_F32 (y_f8 / y2_f8 ignored, no dst_mode / y2): y as above, and with
 * epi->stats the per-channel sums and sums of squares of the fp32 values, row p over the pixels [128 p, 128 p + 128) --
 * every row written, fixed summation order, no atomics; stats_rows must equal the query below, stats_ld >= round_up(cout,
 * 256).  Both MCAMD_Q8_MFMA forms, both `pad` forms of x, any batch size. */
int32_t mcamd_conv_fwd_q8_stats_rows(const mcamd_conv_geom* g);   /* 0 when the geometry has no fp8 form */
/* w_q = deq(q(w * mask * 2^e_f)) * 2^-e_f as fp32 OIHW [cout][cin][k][k], e_f = wexp[f] as mcamd_pack_q8 wrote it for the same
 * weights and mask: the values the forward's weight bytes stand for.  mcamd_pack_weights(_many) builds the dgrad operand
 * from it (with no mask). */
int mcamd_fakequant_q8(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, const int32_t* wexp,
                       float* wq_oihw, void* stream);
/* mcamd_cast_q8 that also writes deq(code) / 2 (exact in fp16) back over the source slice. */
int mcamd_cast_q8_train(void* src, int64_t pixels, int32_t src_ld, int32_t src_choff, int32_t C, void* dst, int32_t dst_ld,
                        int32_t dst_choff, void* stream);

/* ---------------------------------------------------------------------------
 * 2:4-sparse fp8 quantised inference (an addition beyond the reference; conv_q8_sparse.hip, Darknet.precision =
 * "fp8-2:4"): the fp8 block above -- same activations, exponents, q(), output formula and destinations -- for weights
 * whose mask keeps at most 2 of every 4 consecutive input channels at each (filter, tap), on the sparse MFMA.  S is an fp32
 * sum of the exact products (v_smfmac_f32_32x32x32_f16 on the bytes converted in registers); MCAMD_Q8_MFMA=1 multiplies on
 * v_smfmac_f32_32x32x64_fp8_fp8 instead, which like the dense fp8 MFMA truncates inside groups of 8 products.
 * ------------------------------------------------------------------------- */
/* mcamd_conv_fwd_q8_ok's predicate (cin % 64 == 0 implies whole groups of 4). */
int32_t mcamd_conv_fwd_q8_sparse24_ok(const mcamd_conv_geom* g);
/* Sizes of the packed operands: out[0] = kept bytes (Npad * ktot / 2; Npad = round_up(cout, 256), ktot = k*k * cin),
 * out[1] = 32-bit index words (Npad * ktot / 32), out[2] = int32 exponents (Npad). */
int mcamd_q8_sparse24_elems(const mcamd_conv_geom* g, int64_t out[3]);
/* OIHW fp32 master (* mask, may be NULL) -> the 2:4 fp8 packing:
 *   wexp: int32 [Npad], e_f of mcamd_pack_q8 (from max |w * mask| over the WHOLE filter; pad rows 0);
 *   wq:   bytes [Npad][ktot / 2]: the dense row of mcamd_pack_q8 (position kpos(t, c) = (c / 64) * k*k*64 + t * 64 + c % 64)
 *         with every group of 4 consecutive positions [4 G, 4 G + 4) -- 4 consecutive input channels at one tap -- reduced
 *         to its 2 kept bytes: kept byte j of the row (j < ktot / 2) belongs to group G = j / 2; pad rows zero bytes;
 *   idx:  uint32 [ktot / 64][Npad][2]: word idx[(q * Npad + n) * 2 + h] describes kept bytes j in [32 q + 16 h, +16) of row
 *         n; bits [2 i, 2 i + 2), i = j - 32 q - 16 h, hold the offset o of kept byte j inside its group: its dense position
 *         is 4 (j / 2) + o.  The two offsets of a group are distinct and ascending.
 * The kept entries of a group are the non-zeros of the fp32 product w * mask in channel order (the first two when the mask
 * does not conform); a group with fewer gets distinct ascending offsets with zero values (none: 0, 1; one at offset o: (o, o
 * + 1) if o == 0 else (0, o)).  The bytes are q(kept value * 2^e_f).  Every row up to Npad is written. */
int mcamd_pack_q8_sparse24(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* wq, void* idx,
                           int32_t* wexp, void* stream);
/* mcamd_conv_fwd_q8 from that packing (the same arguments plus `idx`). */
int mcamd_conv_fwd_q8_sparse24(const mcamd_conv_geom* g, const void* x8, const void* wq, const void* idx, const int32_t* wexp,
                               const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, void* stream);

/* ---------------------------------------------------------------------------
 * 4-bit weight inference on the fp8 engine (an addition beyond the reference; conv_q8_w4.hip, Darknet.precision =
 * "fp8-w4"): the fp8 block above -- same activations, q(), output formula and destinations -- with the weights
 * held as 4-bit e2m1 codes and one shift per group of 32 input channels: 4.25 bits per weight.  Per filter f of
 * w = weight * mask, with e_f as mcamd_pack_q8 computes it:
 *   filter exponent  e4_f = e_f - 1 (0 for an all-zero filter); s = w * 2^e4_f: the filter's largest |s| lies in (112, 224];
 *   groups           the 32 consecutive input channels [32 j, 32 j + 32) at one tap of one filter (cin % 64 == 0: every 64-k
 *                    chunk of the packed order holds exactly two);
 *   group shift      the smallest integer g in [-5, 6] with max |s| over the group <= 6 * 2^g ((m, x) = frexp(max): x - 3 if
 *                    m <= 0.75 else x - 2, clamped); -5 for an all-zero group;
 *   code             bit 3 = sign, bits 0-2 = index into {0, 0.5, 1, 1.5, 2, 3, 4, 6} of |s| / 2^g rounded to nearest, ties to
 *                    the index with the even mantissa bit (2.5 -> 2, 3.5 -> 4, 5 -> 4, 0.25 -> 0); a zero magnitude has no sign
 *                    bit (the packer writes no -0; the kernels read one as 0).  Groups below 0.25 * 2^-5 come out as zeros;
 *   value            grid[code] * 2^g.  Every such value is an e4m3 number (one mantissa bit, 2^-6 <= |value| <= 384 <= 448), so
 *                    its byte W8x = q(value) is exact, and
 *   output           v = leaky(scale_f * 2^-(e4_f + 1) * S + shift_f), S = sum a8 * W8x: mcamd_conv_fwd_q8 on the bytes W8x
 *                    with the exponents e4_f, bit for bit, in both MCAMD_Q8_MFMA forms (the kernel expands the codes to those
 *                    bytes in registers and issues that kernel's MFMA sequence).
 * ------------------------------------------------------------------------- */
/* mcamd_conv_fwd_q8_ok's predicate. */
int32_t mcamd_conv_fwd_q8_w4_ok(const mcamd_conv_geom* g);
/* Sizes of the packed operands: out[0] = code bytes (Npad * ktot / 2; Npad = round_up(cout, 256), ktot = k*k * cin),
 * out[1] = shift bytes (Npad * ktot / 32), out[2] = int32 exponents (Npad). */
int mcamd_q8_w4_elems(const mcamd_conv_geom* g, int64_t out[3]);
/* OIHW fp32 master (* mask, may be NULL) -> the 4-bit packing, everything computed on the device, no atomics:
 *   wexp:   int32 [Npad], e4_f (pad rows 0);
 *   gshift: bytes [ktot / 64][Npad][2]: gshift[(q * Npad + n) * 2 + j] = g + 5 of group j of chunk q of row n -- the positions
 *           kpos in [64 q + 32 j, +32) of mcamd_pack_q8's order kpos(t, c) = (c / 64) * k*k*64 + t * 64 + c % 64; pad rows 0;
 *   codes:  bytes [Npad][ktot / 2]; chunk q of row n is the 32 bytes [32 q, 32 q + 32), two 16-byte pieces h = 0, 1 (one lane's
 *           operand each).  Piece h holds the chunk's positions p(h, t), t in [0, 32): p = 16 h + t for t < 16 (group 0),
 *           32 + 16 h + (t - 16) otherwise (group 1).  Byte i of the piece, with d = i / 4, b = i % 4: the low nibble is the
 *           code of t = 8 d + b, the high nibble the code of t = 8 d + 4 + b.  Pad rows: zero codes.
 * Every row up to Npad is written. */
int mcamd_pack_q8_w4(const mcamd_conv_geom* g, const float* w_oihw, const float* mask_oihw, void* codes, void* gshift,
                     int32_t* wexp, void* stream);
/* codes + gshift -> wq: the e4m3 bytes W8x, [Npad][ktot] in exactly mcamd_pack_q8's layout (pad rows zero bytes):
 * mcamd_conv_fwd_q8(.., wq, wexp = e4_f, ..) then computes what mcamd_conv_fwd_q8_w4 computes. */
int mcamd_unpack_q8_w4(const mcamd_conv_geom* g, const void* codes, const void* gshift, void* wq, void* stream);
/* mcamd_conv_fwd_q8 from that packing: epi->mode MCAMD_EPI_PAD_F16 only; dst_mode, y2, y_f8 / y2_f8 as there.  Both
 * MCAMD_Q8_MFMA forms, both `pad` forms of x, any batch size. */
int mcamd_conv_fwd_q8_w4(const mcamd_conv_geom* g, const void* x8, const void* codes, const void* gshift, const int32_t* wexp,
                         const mcamd_conv_epilogue* epi, int32_t y_f8, int32_t y2_f8, void* stream);
/* The kernel instance mcamd_conv_fwd_q8_w4 launches for this geometry (host logic only): out as mcamd_conv_fwd_q8_info's --
 * the tile mcamd_conv_fwd_q8 takes for the same geometry (no instance needs scratch memory, none is left out). */
int mcamd_conv_fwd_q8_w4_info(const mcamd_conv_geom* g, int32_t out[7]);

/* ---------------------------------------------------------------------------
 * 4-bit quantisation-aware training (an addition beyond the reference; Darknet.precision = "fp8-w4-qat"): the
 * fp8 quantisation-aware training above with the weights of every fp8 block in the 4-bit format above -- the training-mode
 * forward of a block runs on the codes it would be deployed with under "fp8-w4".
 *   forward   a8 = q(2 x) input codes, as there; every step w = weight * mask is re-quantised on the device by
 *             mcamd_pack_q8_w4 into codes, group shifts g and filter exponents e4_f (the format is unchanged);
 *             raw output y[m][f] = 2^-(e4_f + 1) * sum a8 * W8x, fp32 [B*H*W][y_ld], W8x the e4m3 bytes the codes stand for --
 *             the convolution of x_q = deq(a8) / 2 with w_q = grid[code] * 2^g * 2^-e4_f (the powers of two are exact);
 *             the BatchNorm statistics of those fp32 values, the coefficients, the byte and fp16-twin stores and the
 *             fp16 -> fp8 edge are exactly those of "fp8-qat".
 *   backward  straight-through, WITHOUT a clipping mask: dX = dgrad(dY, fp16(w_q)), dW = wgrad(dY, x_q) * mask, master
 *             weights fp32.  A weight its group rounds to code 0 still receives its gradient.  fp16(w_q) is exact whenever
 *             w_q stays in fp16's normal range (one mantissa bit).
 *   An inference-mode forward under "fp8-w4-qat" is the "fp8-w4" engine's, bit for bit.
 * ------------------------------------------------------------------------- */
/* mcamd_conv_fwd_q8_w4's K loop (staging, register decode, both MCAMD_Q8_MFMA forms) with mcamd_conv_fwd_q8's
 * MCAMD_EPI_RAW_F32 epilogue -- the only mode accepted: y as above and, with epi->stats, the per-channel sums and sums of squares
 * of the fp32 values, row p over the pixels [128 p, 128 p + 128) -- every row written, fixed summation order, no atomics;
 * stats_rows must equal mcamd_conv_fwd_q8_stats_rows(g), stats_ld >= round_up(cout, 256).  Bit-equal to mcamd_conv_fwd_q8 in that
 * mode on mcamd_unpack_q8_w4's bytes with the exponents e4_f.  The tile is the one mcamd_conv_fwd_q8 takes in that mode
 * (mcamd_conv_fwd_q8_info, form 1).  Both `pad` forms of x, any batch size. */
int mcamd_conv_fwd_q8_w4_raw(const mcamd_conv_geom* g, const void* x8, const void* codes, const void* gshift, const int32_t* wexp,
                             const mcamd_conv_epilogue* epi, void* stream);
/* w_q = grid[code] * 2^g * 2^-e4_f as fp32 OIHW [cout][cin][k][k], decoded from mcamd_pack_q8_w4's operands through the layout
 * stated above: the values the forward multiplied.  A masked weight has code 0 and comes out as exactly 0.
 * mcamd_pack_weights(_many) builds the dgrad operand from it (with no mask). */
int mcamd_fakequant_q8_w4(const mcamd_conv_geom* g, const void* codes, const void* gshift, const int32_t* wexp, float* wq_oihw,
                          void* stream);

/* dx = conv_transpose(dy, w) -- autograd's input gradient of the same call.
 * `dy` is padded NHWC fp16 [B][H+2][W+2][dy_ld] (zero halo); g->cin/cout keep their forward
 * meaning; the result has g->cin channels.  epi->mode 0 (fp16 [M][y_ld]) or 1 (fp32 NCHW). */
int mcamd_conv_dgrad(const mcamd_conv_geom* g, const void* dy, int32_t dy_ld, int32_t dy_choff,
                     const void* wp_dgrad, const mcamd_conv_epilogue* epi, void* stream);

/* The same launch, also taking the sums of the BatchNorm backward of the PLAIN block (BatchNorm + LeakyReLU, nothing
 * pooled or reorg'ed behind it; nn.BatchNorm2d + nn.LeakyReLU under autograd, reference src/nets.py:802-809) whose
 * output gradient G it stores: the tile is in LDS as fp16 on its way out, the block's stored activation at the same pixel
 * and channel is this convolution's own forward input, so sum g_z and sum g_z xhat per channel -- the first pass of
 * mcamd_bn_act_bwd with mcamd_act_bwd_desc.act, same formulas, same ill-conditioned-channel rule, on G AS STORED -- are
 * formed here and mcamd_bn_act_bwd (mcamd_act_bwd_desc.sums) skips that pass.  Fixed summation order, no atomics.
 * `sums` NULL (or sums->slab NULL): exactly mcamd_conv_dgrad. */
typedef struct mcamd_dgrad_sums {
    float* slab;               /* out: fp32 [rows][2][ld]; every row and every producer channel is written */
    int32_t rows;              /* must equal mcamd_conv_dgrad_sums_rows(geom, epilogue.concurrent) */
    int32_t ld;                /* >= C */
    const void* act;           /* the producer's stored fp16 activation, as mcamd_act_bwd_desc.act: padded NHWC (act_pad 1:
                                  shared-halo form) at this geometry's B, H, W, producer channel c at act_choff + c of act_ld */
    int32_t act_ld, act_choff, act_pad;
    const float* scale; const float* shift; const float* mean; const float* invstd;   /* the producer's, [C] */
    float slope;               /* the producer's negative-side slope (> 0) */
    const float* y;            /* the producer's saved fp32 raw output [B*H*W][y_ld] (channels from y_choff) or NULL: read
                                  for ill-conditioned channels only, as mcamd_act_bwd_desc.y with `act` */
    int32_t y_ld, y_choff;
    int32_t ch_lo, C;          /* the producer's C channels are channels [ch_lo, ch_lo + C) of this launch's output
                                  (multiples of 8; a concat member: its offset inside the consumer's input slice) */
} mcamd_dgrad_sums;
/* Slab rows such a launch writes, from the route function the launch asks; 0: the kernel this geometry gets cannot take
 * sums (the caller keeps the two-pass mcamd_bn_act_bwd). */
int32_t mcamd_conv_dgrad_sums_rows(const mcamd_conv_geom* g, int32_t concurrent);
int mcamd_conv_dgrad_sums(const mcamd_conv_geom* g, const void* dy, int32_t dy_ld, int32_t dy_choff,
                          const void* wp_dgrad, const mcamd_conv_epilogue* epi, const mcamd_dgrad_sums* sums, void* stream);

/* dW = wgrad(x, dy) * mask / grad_scale, written as fp32 OIHW -- autograd's weight gradient of
 * `self.weight * mask_var` followed by F.conv2d.  Deterministic (slab reduction, no atomics).
 * Fully pruned filters are skipped through `map` (may be NULL): the caller keeps the surviving filters first
 * in its channel order and passes a geometry whose `cout` is the kept count, so that forward, dgrad and
 * wgrad all run on the kept filters only (modelcompression_amd/engine.py, "filter compaction").  With a map,
 * dW[rows[n]][cols[c]] receives the gradient of physical (n, c) (the mask is read at the same place) and
 * tensor rows that are not in rows[] are NOT written: the caller zeroes dw_oihw first.
 * `dbias` (fp32[cout], may be NULL) receives sum over pixels of dy / grad_scale. */
size_t mcamd_conv_wgrad_workspace_bytes(const mcamd_conv_geom* g);
int mcamd_conv_wgrad(const mcamd_conv_geom* g, const void* x, const void* dy, int32_t dy_ld,
                     int32_t dy_choff, const float* mask_oihw, const mcamd_chan_map* map,
                     float grad_scale, float* dw_oihw, float* dbias, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Which kernels mcamd_conv_wgrad launches for this geometry (has_cmap != 0: with map->cols), from the plan and decision
 * functions the launch itself calls; works without a GPU.  out[]:
 *   0     family: MCAMD_WGRAD_GENERIC wgrad_kernel<TMo, TNc, TAPS, KP, NS>, _STEM wgrad_stem_kernel<NS>, _WIN
 *         wgrad_win_kernel<TMo / 32, NS>, _NINE wgrad9_kernel<KP>, _NINE_WIDE wgrad9w_kernel<KP, NS>
 *   1-5   TMo, TNc, TAPS, KP, NS: filters x input channels x taps of a workgroup, pixels per step, LDS ring stages
 *   6-8   nsplit (pixel splits = fp32 slabs), pix_per_split (0: the stem / win kernels divide the steps themselves),
 *         rows_pad (filter rows of a slab; the dy slice that is read is that wide)
 *   9-10  finish kernel: MCAMD_WFIN_ROW wgrad_finish_row_kernel<k*k> (SG 0), _VEC wgrad_finish_vec_kernel<k*k, SG>,
 *         _GENERIC wgrad_finish_kernel<SG>; and SG (1 / 8 / 32)
 *   11-12 tiles (workgroups per split) and workgroups launched (tiles * nsplit, rounded up to 8 where the kernel asks it) */
#define MCAMD_WGRAD_GENERIC 0
#define MCAMD_WGRAD_STEM 1
#define MCAMD_WGRAD_WIN 2
#define MCAMD_WGRAD_NINE 3
#define MCAMD_WGRAD_NINE_WIDE 4
#define MCAMD_WFIN_ROW 0
#define MCAMD_WFIN_VEC 1
#define MCAMD_WFIN_GENERIC 2
#define MCAMD_WGRAD_PLAN_INFO_N 13
int mcamd_conv_wgrad_plan_info(const mcamd_conv_geom* g, int32_t has_cmap, int32_t out[MCAMD_WGRAD_PLAN_INFO_N]);
/* The (TMo, TNc, TAPS, KP) of every wgrad_kernel instance the library holds, 4 values each; at most `cap` tuples are
 * written (out may be NULL with cap 0); returns their number.  Any other tuple is an MCAMD_EINVAL of the launch. */
int32_t mcamd_wgrad_generic_instances(int32_t* out, int32_t cap);

/* ------------------------------------------------------------------------- *
 * The list launch of the weight gradient (Darknet.sparse_train = "block-wgrad").  For a block mask the zero
 * blocks of dW are OUTPUT tiles of the two 64 x 64 weight-gradient kernels: a block of 64 filters x 64 input channels x one
 * tap (block_prune) is one tap of a wgrad9_kernel workgroup tile (3x3 layers) or a whole tile of wgrad_kernel<64, 64, 1, 64>
 * (1x1 layers).  The launch runs the listed tiles only, and of a 3x3 tile the taps whose bit is set in its tap word; the
 * finish pass writes exactly 0.0f wherever the mask is zero WITHOUT reading the slabs there (skipped tiles and taps leave
 * their part of the workspace as it was), and sum * (1 / grad_scale) * mask elsewhere, in mcamd_conv_wgrad's order of
 * additions.  The lists come from the MASK, never from weight values: a kept weight that is zero still has a gradient.  Any
 * mask is correct, block-aligned or not: a tile or tap is kept when any of its mask elements is non-zero (-0 counts as
 * zero), and an elementwise hole inside a kept block is the finish pass's select.  Deterministic; no atomics on floats.
 * ------------------------------------------------------------------------- */
/* 1: ksize 1 or 3, stem == 0, x_wrap == 0, x_f8 == 0, cin % 64 == 0, cout % 64 == 0, the input slice inside x_ld, and for
 * ksize 3 the geometries of the padded-pixel 9-tap kernel (W <= 208 and the MCAMD_WGRAD9 switch on).  Host logic only. */
int32_t mcamd_conv_wgrad_bsparse_ok(const mcamd_conv_geom* g);
/* int32 entries of the lists: out[0] = the tiles nt = (cout / 64) * (cin / 64) (tile list), out[1] = 2 nt (tap words). */
int mcamd_wgrad_bsparse_elems(const mcamd_conv_geom* g, int64_t out[2]);
/* From the fp32 OIHW mask: the word of tile (ot, ct), index ot * (cin / 64) + ct, has bit t set iff any mask element of
 * filters [64 ot, 64 ot + 64) x channels [64 ct, 64 ct + 64) x tap t is non-zero (ksize 1: bit 0).  tiles[0 .. counts[0]):
 * the tiles with a non-zero word, ascending; words[0 .. counts[0]): their words; counts[1]: the kept (tile, tap) pairs.
 * Entries behind counts[0] are written as 0; words[nt .. 2 nt) holds the word of EVERY tile.  No host synchronisation. */
int mcamd_wgrad_bsparse_lists(const mcamd_conv_geom* g, const float* mask_oihw, int32_t* tiles, int32_t* words, int32_t* counts,
                              void* stream);
/* What a list launch of `kept_tiles` tiles runs (host logic only, the launch's own plan function): out = {family
 * (MCAMD_WGRAD_NINE wgrad9_kernel<KP>, never the wide form; MCAMD_WGRAD_GENERIC wgrad_kernel<64, 64, 1, 64>), KP, LDS ring
 * stages, nsplit, pix_per_split, finish kernel (MCAMD_WFIN_VEC: its select form), SG, workspace bytes}.  nsplit is
 * mcamd_conv_wgrad's cost rule applied to the kept tile count (0 tiles count as one). */
#define MCAMD_WGRAD_BSPARSE_PLAN_N 8
int mcamd_conv_wgrad_bsparse_plan(const mcamd_conv_geom* g, int32_t kept_tiles, int64_t out[MCAMD_WGRAD_BSPARSE_PLAN_N]);
/* dw_oihw and dbias as mcamd_conv_wgrad computes them with the same mask (no channel map), on the `ntiles` listed tiles.
 * `nsplit` is the caller's (from the plan query: 1 .. the steps of the kernel), so that a launch on full lists -- every tile,
 * word 0x1ff or 1 -- runs at the split count of the short ones and gives the same bits; workspace >= nsplit * cout * k*k *
 * cin floats (out[7] above).  ntiles == 0 launches the finish pass only: all zeros.  `words` may be NULL for ksize 1.  A
 * tile index outside [0, nt) is skipped.  The mask must be the one the lists were built from: a kept element outside the
 * listed tiles and taps would read slab that nobody wrote. */
int mcamd_conv_wgrad_bsparse(const mcamd_conv_geom* g, const void* x, const void* dy, int32_t dy_ld, int32_t dy_choff,
                             const float* mask_oihw, const int32_t* tiles, const int32_t* words, int32_t ntiles, int32_t nsplit,
                             float grad_scale, float* dw_oihw, float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* The whole backward of a dense 1x1 block in ONE launch plus the weight gradient's finish pass: what mcamd_conv_dgrad_sums
 * (epilogue mode 0) and mcamd_conv_wgrad compute for the same arguments, from one pass over dY and x.
 *   gin[m][g_choff + c] = sum_n dy[m][n] w[n][c] as fp16 [B*H*W][g_ld], saturated to +-65504 with `overflow` (may be NULL)
 *                          set to 1 where a value was clamped, exactly as mcamd_conv_dgrad stores it; nothing else of gin is
 *                          written;
 *   `sums` (may be NULL): the BatchNorm-backward sums of the PLAIN block that produced x, as mcamd_conv_dgrad_sums forms them
 *                          -- sums->rows = mcamd_conv_bwd1x1_sums_rows(g), every row and every producer channel written; the
 *                          producer's stored activation must BE this block's input (act == x, act_ld == g->x_ld, act_choff ==
 *                          g->x_choff + ch_lo, act_pad == g->pad): the launch reads it from the tile of x it holds on chip;
 *   dw_oihw = dy^T x * mask / grad_scale, dbias as mcamd_conv_wgrad (no channel map); workspace >=
 *                          mcamd_conv_bwd1x1_workspace_bytes(g): one fp32 [cout][cin] split per workgroup
 *                          (mcamd_conv_bwd1x1_wgrad_splits of them), summed by mcamd_conv_wgrad's finish kernel.
 * A persistent launch of a fixed grid; no workgroup waits for another, no atomics on results: two runs give the same bits.
 * mcamd_conv_bwd1x1_ok (host logic only): 1 when the geometry has such a launch -- ksize 1, no stem / x_wrap / x_f8, an
 * existing (cout, cin) instance: (64, 128), (128, 256), x slice in whole groups of 8 -- else 0 with *reason (may be NULL)
 * pointing at a static string that says why; the launch returns MCAMD_EINVAL with the same reason.  The three queries
 * return 0 for a refused geometry.  Both `pad` forms of x and dy. */
int32_t mcamd_conv_bwd1x1_ok(const mcamd_conv_geom* g, const char** reason);
int32_t mcamd_conv_bwd1x1_sums_rows(const mcamd_conv_geom* g);
int32_t mcamd_conv_bwd1x1_wgrad_splits(const mcamd_conv_geom* g);
size_t mcamd_conv_bwd1x1_workspace_bytes(const mcamd_conv_geom* g);
int mcamd_conv_bwd1x1(const mcamd_conv_geom* g, const void* x, const void* dy, int32_t dy_ld, int32_t dy_choff,
                      const void* wp_dgrad, void* gin, int32_t g_ld, int32_t g_choff, int32_t* overflow,
                      const mcamd_dgrad_sums* sums, const float* mask_oihw, float grad_scale, float* dw_oihw, float* dbias,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * BatchNorm2d (eps, momentum as given; torch defaults 1e-5 / 0.1 at nets.py:802)
 * + LeakyReLU(0.1) (nets.py:809) + MaxPool2d(2,2) (nets.py:821) + Reorg(2)
 * (nets.py:648-667) + route/concat (nets.py:738-746), fused around the convs.
 * ------------------------------------------------------------------------- */
/* Batch statistics from the conv epilogue's partial sums -> affine coefficients.
 * scale = gamma*invstd, shift = beta - mean*scale.  training != 0: batch stats (biased var),
 * running stats updated with the unbiased var; training == 0: running stats. */
/* `chan_perm` (device int32[C], may be NULL = identity): statistics and the output vectors are in the
 * kernels' physical channel order, gamma/beta/running_* in the module's order; physical channel c reads and
 * updates index chan_perm[c] of them.  The engine keeps the filters that survive filter pruning first (its
 * convolutions then run on the kept filters only) and passes that order here. */
int mcamd_bn_coeffs(const float* stats, int32_t stats_rows, int32_t stats_ld, int32_t C, int64_t count,
                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, int32_t training,
                    float* scale, float* shift, float* save_mean, float* save_invstd,
                    const int32_t* chan_perm, void* stream);

/* As mcamd_bn_coeffs; `ones_channel` >= 0 names ONE physical channel whose coefficients are forced to scale 0 /
 * shift 1 after the statistics update: the BatchNorm + LeakyReLU pass then writes 1.0 at every interior pixel of that
 * channel (0 stays in the halo).  The engine uses the first dead channel behind the kept filters of a filter-pruned
 * layer this way when the consumer folds the dead inputs (mcamd_fold_weights); -1 = none. */
int mcamd_bn_coeffs_ex(const float* stats, int32_t stats_rows, int32_t stats_ld, int32_t C, int64_t count,
                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                       float momentum, float eps, int32_t training,
                       float* scale, float* shift, float* save_mean, float* save_invstd,
                       const int32_t* chan_perm, int32_t ones_channel, void* stream);

#define MCAMD_DST_PLAIN 0  /* same resolution */
#define MCAMD_DST_POOL 1   /* 2x2/2 max pool */
#define MCAMD_DST_REORG 2  /* reorg stride 2: out channel = (hs*2+ws)*C + c at (h/2, w/2) */
typedef struct mcamd_act_desc {
    int32_t B, H, W, C;        /* conv output size */
    const void* y; int32_t y_ld, y_choff;   /* raw conv output fp16 [B*H*W][y_ld] */
    const float* scale; const float* shift; /* per channel */
    float slope;               /* 0.1 (leaky) or 1.0 (linear) */
    int32_t mode;              /* MCAMD_DST_* for dst */
    void* dst; int32_t dst_ld, dst_choff;   /* padded NHWC fp16 at the mode's resolution */
    void* dst2; int32_t dst2_ld, dst2_choff;/* optional second copy, PLAIN resolution (route of a pooled layer) */
    int32_t y_dtype;           /* 0: y is fp16 (MCAMD_EPI_RAW_F16), 1: y is fp32 (MCAMD_EPI_RAW_F32) */
    int32_t planes;            /* 1 (0 is read as 1), or 3 = split storage for the "fp16x3" precision mode: the
                                  activation v is written as the fp16 pair hi = fp16(v), lo = fp16(v - hi) plus a second
                                  copy of hi, at channels choff + {0, 1, 2} * plane stride.  A convolution whose input
                                  is the 3*C-channel run [hi | lo | hi] and whose packed weights are [w_hi | w_hi | w_lo]
                                  (w_hi = fp16(w), w_lo = fp16(w - w_hi)) accumulates x_hi*w_hi + x_lo*w_hi + x_hi*w_lo
                                  in fp32 on the fp16 MFMA path: operand rounding drops from 2^-11 to ~2^-21, which
                                  is what the reference's fp32 F.conv2d (layers.py:60-64) needs over 23 layers for
                                  1e-3 logits (tools/error_budget.py).  Reading channels [0, C) alone is the plain
                                  fp16 activation.
                                  2 = hi and lo only: the consumer reads the hi plane twice (mcamd_conv_geom.x_wrap),
                                  4 instead of 6 bytes written per activation.
                                  4 = hi and, one plane stride further, the e4m3 correction bytes [lo8 | x8] of a consumer
                                  with mcamd_conv_geom.x_f8 (each `plane` BYTES long; fp32 y only). */
    int32_t dst_plane, dst2_plane; /* plane strides (channels, multiples of 8) of dst / dst2 when planes >= 2 */
    int32_t dst_pad, dst2_pad; /* 0 / 1: dst, dst2 are in the padded / the shared-halo form (each at its own resolution) */
    const float* border;       /* optional fp32 [16][C], NULL = none: added to the raw conv output before the
                                  affine step, row = border class of the pixel (bit 0: h == 0, bit 1: h == H-1,
                                  bit 2: w == 0, bit 3: w == W-1).  Physically slim filter-pruned models fold the
                                  constant output of their removed input channels into this table, because zero
                                  padding clips it differently at the borders (BASELINE config 5; the reference
                                  only states slim convs as a conclusion, README.md:19). */
    int32_t planes2;           /* storage form of dst2 when it differs from dst's (its consumer is another convolution);
                                  0 = `planes` */
    void* pool_act;            /* optional (mode MCAMD_DST_POOL), NULL = none: a FULL-RESOLUTION fp16 copy of the activation,
                                  padded NHWC / shared-halo form per pool_act_pad, pool_act_ld channels per pixel, channels
                                  [0, C) -- what mcamd_bn_act_bwd reads instead of the raw output (mcamd_act_bwd_desc.act)
                                  in the backward pass of a MaxPool block.  The element the pool took (the first maximum
                                  of the four UNROUNDED activations in (h, w) scan order, nn.MaxPool2d(2, 2), reference
                                  src/nets.py:821) is stored as the STRICT maximum of the window: a neighbour that rounds to
                                  the same fp16 value is written one fp16 step lower (~6e-4 of the elements of a random
                                  tensor), so that the backward pass routes the gradient where the fp32 forward did. */
    int32_t pool_act_ld, pool_act_pad;
    void* dst_q8;              /* optional, NULL = none (fp32 y, planes 1, no pool_act): a BYTE twin of dst -- the same padded form,
                                  resolution, dst_ld (bytes per pixel) and dst_choff, halo bytes 0x00 and never written.  It
                                  receives the e4m3 codes q(2 v) of mcamd_conv_fwd_q8's contract (mode POOL: q of 2 x the window
                                  maximum; REORG: mapped as dst), ONE rounding from fp32, and dst then receives deq(code) / 2
                                  (exact in fp16) instead of fp16(v): the training-mode forward of an fp8 block
                                  (Darknet.precision = "fp8-qat"), whose backward multiplies what the consumer's forward did. */
    void* dst2_q8;             /* the same for dst2 (needs dst2) */
} mcamd_act_desc;
int mcamd_bn_act_fwd(const mcamd_act_desc* d, void* stream);

/* Which kernel instance mcamd_bn_act_fwd launches for a descriptor (host logic only: no GPU work, the pointers are compared
 * with NULL and never read).  The launch and this query ask one function (`act_route` in csrc/bn_act.hip), so the query
 * returns MCAMD_OK exactly where the launch would, and the launch's error (code and mcamd_last_error text) where it refuses.
 *   mode             : MCAMD_DST_* as given
 *   fixed            : 1 when C / 8 divides 256 (a thread keeps one channel group and its coefficients in registers), else 0
 *                      (any C % 8 == 0: coefficients re-read per item)
 *   y32              : 1 for an fp32 y
 *   planes, planes2  : the storage forms of dst and dst2 with the zeros resolved (planes 0 -> 1, planes2 0 -> planes)
 *   q8               : 1 when a byte twin (dst_q8 / dst2_q8) is given
 *   items            : 8-channel groups x pixels at the mode's resolution; grid: workgroups of 256 threads, at most 4096 --
 *                      beyond that a thread takes more than one item
 * The library holds 48 instances: 3 modes x fixed 0/1 x {fp16 y: planes 1, 2, 3; fp32 y: planes 1, 2, 3, 4; q8}. */
typedef struct mcamd_act_instance { int32_t mode, fixed, y32, planes, planes2, q8; int64_t items; int32_t grid; } mcamd_act_instance;
int mcamd_bn_act_fwd_instance(const mcamd_act_desc* d, mcamd_act_instance* out);

/* mcamd_bn_act_fwd(d) followed by mcamd_conv_fwd(g, d->dst, wp_fwd, epi) in ONE launch, for a PLAIN block whose only
 * consumer is a 1x1 convolution on split operands (csrc/bn_conv1x1.hip): a workgroup reads the producer's fp32 raw output
 * d->y once, applies leaky(y * scale + shift), splits into hi = fp16(v) saturated and lo = fp16(v - hi) in registers and
 * multiplies x_hi w_hi + x_lo w_hi + x_hi w_lo with the packed weights [w_hi | w_hi | w_lo] (mcamd_pack_job.split 1) on the
 * fp16 MFMAs -- the same instructions in the same K order as the launches it replaces, so epi->y and epi->stats are
 * BIT-EQUAL to theirs.  The hi plane is still written, to channels [d->dst_choff, d->dst_choff + d->C) of the interior
 * pixels of d->dst (the backward pass reads it); the lo plane and the halo are not touched.  Replaces nn.BatchNorm2d +
 * nn.LeakyReLU + F.conv2d (reference src/nets.py:802-809, src/pruning/weightPruning/layers.py:60-64) for such a pair.
 *   d   : the activation pass as mcamd_bn_act_fwd would get it: mode MCAMD_DST_PLAIN, fp32 y (y_dtype 1), planes 2 with
 *         dst_plane == C, dst_pad 0, no dst2 / border / pool_act / dst_q8
 *   g   : the consumer's forward geometry as mcamd_conv_fwd would get it: ksize 1, cin = 3 C, x_wrap = 2 C, pad 0, no x_f8,
 *         x_ld == d->dst_ld, x_choff == d->dst_choff, the producer's B x H x W
 *   epi : mode MCAMD_EPI_RAW_F32; stats may be NULL (no slab is written), else stats_rows ==
 *         mcamd_bn_act_conv1x1_stats_rows(d, g) (== mcamd_conv_stats_rows_mode(g, MCAMD_EPI_RAW_F32))
 * mcamd_bn_act_conv1x1_ok (host logic only, pointers are not read): 1 when the pair has a fused launch -- the above, C % 64
 * == 0, cout % 8 == 0 within one column tile (<= 128), C <= 128 (cout <= 64) or 256 (a thread keeps its converted values in
 * registers across the three parts), and a consumer whose own forward takes igemm_kernel's 128-pixel tiles of 64 or 128
 * columns (the persistent slots and the wave rows of 64 pixels, hence the slab and its summation order, are that launch's;
 * cout <= 32 takes the 32-column tile there and is refused).  Everything else is refused, by the launch entry too (MCAMD_EINVAL). */
int32_t mcamd_bn_act_conv1x1_ok(const mcamd_act_desc* d, const mcamd_conv_geom* g);
int32_t mcamd_bn_act_conv1x1_stats_rows(const mcamd_act_desc* d, const mcamd_conv_geom* g);   /* 0 when refused */
int mcamd_bn_act_conv1x1_fwd(const mcamd_act_desc* d, const mcamd_conv_geom* g, const void* wp_fwd,
                             const mcamd_conv_epilogue* epi, void* stream);

/* Which kernel instance mcamd_bn_act_conv1x1_fwd launches for a pair, and with which dimensions (host logic only: no GPU
 * work, pointers are not read).  The launch and this query ask one refusal function and one choice function, so the query
 * returns MCAMD_OK exactly where mcamd_bn_act_conv1x1_ok returns 1, and MCAMD_EINVAL with the launch's reason elsewhere.
 *   bn, cb      : bn_conv1x1_kernel<bn, cb> -- the column tile (64 for cout <= 64, else 128) and the 64-channel blocks of
 *                 the producer's C; the library holds <64,1> <64,2> <128,1> <128,2> <128,3> <128,4>
 *   threads     : per workgroup, 4 * bn
 *   rows        : persistent slots = rows of the statistics slab (mcamd_bn_act_conv1x1_stats_rows)
 *   num_mtiles  : tiles of 128 pixels; more tiles than rows: a workgroup takes several
 *   grid        : workgroups launched (rows rounded up to the 8 XCDs, plus one per XCD; the surplus returns at once)
 *   lds_bytes   : dynamic LDS per workgroup */
typedef struct mcamd_bn_conv1x1_instance { int32_t bn, cb, threads, rows, num_mtiles, grid, lds_bytes; } mcamd_bn_conv1x1_instance;
int mcamd_bn_act_conv1x1_info(const mcamd_act_desc* d, const mcamd_conv_geom* g, mcamd_bn_conv1x1_instance* out);

typedef struct mcamd_act_bwd_desc {
    int32_t B, H, W, C;
    const void* y; int32_t y_ld, y_choff;   /* saved raw conv output */
    const float* scale; const float* shift; const float* mean; const float* invstd; /* from mcamd_bn_coeffs */
    float slope;
    int32_t mode;              /* how `g` maps onto this layer's output (MCAMD_DST_*) */
    const void* g; int32_t g_ld, g_choff;   /* fp16 gradient wrt dst, [pixels at mode's resolution][g_ld] */
    const void* g2; int32_t g2_ld, g2_choff;/* optional gradient wrt dst2 (PLAIN resolution) */
    void* dy; int32_t dy_ld, dy_choff;      /* out: padded NHWC fp16 gradient wrt raw conv output */
    float* dgamma; float* dbeta;            /* out fp32 [C], already divided by grad_scale (may be NULL) */
    float grad_scale;          /* the incoming gradients are grad_scale x the true ones (fp16 range) */
    const float* dy_keep;      /* optional fp32 [C]: 0 marks a fully pruned filter; its dY channel is written as
                                  zero (its weights are zero, so dgrad/wgrad never need it -- and a dead filter has
                                  zero batch variance, which would otherwise blow dY up by 1/sqrt(eps)) */
    const int32_t* chan_perm;  /* optional device int32[C]: dgamma / dbeta of physical channel c are written to
                                  index chan_perm[c] (see mcamd_bn_coeffs) */
    int32_t y_dtype;           /* 0: y is fp16, 1: y is fp32 (and the pooled argmax is taken on unrounded activations,
                                  as the split-storage forward keeps them) */
    int32_t* overflow;         /* optional device flag, set to 1 when a dY value was clamped to +-65504 (see
                                  mcamd_conv_epilogue.overflow) */
    int32_t dy_pad;            /* 0 / 1: dy is in the padded / the shared-halo form */
    int32_t skip_dead_param_grads; /* n > 0: dgamma / dbeta of the physical channels c >= n are NOT written -- the
                                  consumer that folded those dead channels delivers their gradients
                                  (mcamd_unfold_wgrad) and `g` holds nothing for them; 0 = write all */
    const void* act;           /* optional, PLAIN blocks without g2: the activation the forward pass stored for the consumer
                                  (fp16, padded NHWC / shared-halo form per act_pad, the hi plane of split storage) at channels
                                  [act_choff, act_choff + C) of rows of act_ld.  LeakyReLU is invertible: z = act > 0 ? act :
                                  act / slope, xhat = (z - beta) / gamma.  The fp16 rounding of act puts up to 2^-11 (|xhat| +
                                  |beta / gamma|) into that xhat, so an ILL-CONDITIONED channel, |gamma| < 2^-5 max(|beta|, 1)
                                  (gamma == 0 included; BN_ACT_T in csrc/bn_act.hip), takes xhat = (y - mean) invstd from `y`
                                  (fp32, y_dtype 1) in both passes; `y` is read only by the threads that hold such a channel.
                                  `y` NULL: those channels use the activation like all others (gamma == 0: dgamma written as
                                  0; |gamma| small: xhat as recovered).  With an fp32 `y` (split-operand precisions) the
                                  two passes read half the bytes; the result carries the fp16 rounding of the stored
                                  activation, as every backward tensor does (nn.BatchNorm2d + nn.LeakyReLU backward,
                                  reference src/nets.py:802-809 under autograd).
                                  Mode MCAMD_DST_POOL (with or without g2): `act` is the FULL-RESOLUTION fp16 copy of the block's
                                  activation the forward pass wrote as mcamd_act_desc.pool_act (H x W, act_choff 0); the
                                  window's argmax is the maximum of the four stored values (strict by construction there)
                                  and every element's LeakyReLU side is the sign of its stored value (ill-conditioned channels
                                  as above: xhat from `y`, argmax and side from the copy) (nn.MaxPool2d(2, 2)
                                  backward, reference src/nets.py:821). */
    int32_t act_ld, act_choff, act_pad;
    const void* pool_out;      /* optional (mode MCAMD_DST_POOL, no g2, with `act` or an fp32 `y`), NULL = none: the POOLED activation the forward
                                  pass stored for the consumer (fp16, H/2 x W/2, padded NHWC / shared-halo form per
                                  pool_out_pad, the hi plane of split storage) at channels [pool_out_choff, pool_out_choff + C)
                                  of rows of pool_out_ld.  Only the pooled element of a window has a gradient, and its stored
                                  value -- the strict maximum of the window's four `act` values -- is this tensor bit for
                                  bit (both are the saturated fp16 rounding of the same maximum), so the pass that forms
                                  the two per-channel sums reads it and `g` (4 bytes per window) instead of the four `act`
                                  values and `g` (10 bytes).  The threads that hold an ill-conditioned channel (see `act`)
                                  still read the window of `act` for the argmax and `y` at it.  dY is formed as without
                                  it.  WITHOUT `act` (fp32 `y`, y_dtype 1): the pass reads 4 bytes per window instead of the
                                  four fp32 `y` values and `g` (18 bytes); xhat = (z - beta) / gamma then comes from the fp16
                                  pooled activation, as `act` gives it for a PLAIN block, and the ill-conditioned channels
                                  take the argmax from the unrounded activations of `y`.  An fp16 `y` is refused: it is the
                                  tensor whose statistics the forward pass took, its xhat is exact.
                                  MCAMD_BN_POOL_SUMS_POOLED=0 ignores the pointer. */
    int32_t pool_out_ld, pool_out_choff, pool_out_pad;
    const float* sums;         /* optional (PLAIN blocks without g2, with `act`), NULL = none: the per-channel sums of the pass
                                  that forms them are ALREADY in this slab -- fp32 [sums_rows][2][sums_ld], row p holding sum g_z
                                  (index 0) and sum g_z xhat (index 1) of a part of the pixels -- written by the dgrad launch
                                  that stored `g` (mcamd_conv_dgrad_sums below).  The call then runs the coefficient kernel and
                                  the dY pass only: one read of `g` and `act` less. */
    int32_t sums_rows, sums_ld;
} mcamd_act_bwd_desc;
size_t mcamd_bn_act_bwd_workspace_bytes(const mcamd_act_bwd_desc* d);
int mcamd_bn_act_bwd(const mcamd_act_bwd_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Dead INPUT channels of a filter-pruned network (csrc/fold.hip).  A fully pruned filter
 * feeds its consumer the constant leaky(beta) (0 in the halo); all such channels together
 * act like ONE channel of ones convolved with the folded filter sum_c leaky(beta_c) W[n][c].
 * The engine runs the consumer's forward / dgrad / wgrad on the producer's kept channels + that
 * one channel with the augmented weights built by mcamd_fold_weights, and maps the augmented
 * weight gradient back with mcamd_unfold_wgrad (which also yields dbeta of the producer's dead
 * channels).  Exact on the reference's semantics: F.conv2d(x, weight * mask) at layers.py:59-64
 * and the BatchNorm / LeakyReLU / MaxPool of nets.py:798-821 between the two convolutions.
 *   w, mask : the consumer's OIHW fp32 master [cout_t][cin_t][k][k] and mask (or NULL)
 *   rows    : device int32[n] physical filter -> tensor row (NULL = identity; n = filters computed)
 *   cols    : device int32[cin_t] physical input channel -> tensor column, kept channels first
 *             (NULL = identity); the first cin_k are taken as they are, the rest are folded
 *   beta    : the PRODUCER's BatchNorm bias in the module's channel order, fp32[cin_t]
 *   waug / dwaug : fp32 [n][cin_aug][k][k], cin_aug >= cin_k + 1 (the convolution kernels want a channel count
 *             that is a multiple of 8): column cin_k is the folded filter, the columns behind it are zero
 * ------------------------------------------------------------------------- */
typedef struct mcamd_fold_desc {
    const float* w; const float* mask;
    const int32_t* rows; const int32_t* cols;
    const float* beta; float slope;
    int32_t n, cin_t, cin_k, cin_aug, ksize;
} mcamd_fold_desc;
int mcamd_fold_weights(const mcamd_fold_desc* d, float* waug, void* stream);
/* Every folding layer of a network in ONE launch (the per-step rebuild of engine.py): `jobs_dev` is a DEVICE array of
 * `njobs` descriptors; first_block = sum of d.n over the preceding jobs, total_blocks = sum over all jobs. */
typedef struct mcamd_fold_job {
    mcamd_fold_desc d;
    float* waug;
    int64_t first_block;
} mcamd_fold_job;
int mcamd_fold_weights_many(const mcamd_fold_job* jobs_dev, int32_t njobs, int64_t total_blocks, void* stream);
/* dw_oihw rows outside rows[] are not written (the caller zeroes them).  prod_dbeta / prod_dgamma: the producer's
 * gradient vectors in the module's order; dead channels receive dbeta (`accumulate` != 0: added to what an earlier
 * consumer of the same producer wrote) and dgamma = 0. */
int mcamd_unfold_wgrad(const mcamd_fold_desc* d, const float* dwaug, float* dw_oihw, float* prod_dbeta,
                       float* prod_dgamma, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------- *
 * The first block as ONE unit: conv1 (3 -> 32 filters, 3x3) + BatchNorm2d + LeakyReLU
 * + MaxPool2d(2,2) (reference src/nets.py:798-821 for the first [convolutional] +
 * [maxpool] pair of yolov2-voc.cfg, F.conv2d at layers.py:60-64) without the block's
 * full-resolution tensors: neither the raw conv output (709 MB at B=64) nor its
 * gradient ever exists in HBM.  Batch statistics come from the 27x27 Gram matrix of
 * the image windows (y = W v is linear in the 27-value window v), the forward pass
 * recomputes nothing, the backward pass recomputes y from the image and reduces the
 * weight gradient algebraically (csrc/conv_stem_block.hip).  Deterministic.
 *   x      : stem input, padded NHWC4 fp16 (as mcamd_conv_geom.stem)
 *   wp     : packed stem weights from mcamd_pack_weights (mask already applied)
 *   dst    : pooled output, padded NHWC fp16 [B][H/2+2][W/2+2][dst_ld], pixel (0,0,0)
 *   g      : gradient wrt dst, fp16 [B*(H/2)*(W/2)][g_ld], grad_scale x the true one
 * Requires W % 32 == 0 and an even H.  `workspace` (mcamd_stem_block_workspace_bytes())
 * carries S and W*C from a training-mode forward call to the backward call of the same
 * step: the caller must not touch it in between.
 * training != 0: batch statistics -> scale/shift/save_mean/save_invstd are WRITTEN and the
 * running statistics updated; training == 0: scale/shift are READ (mcamd_bn_coeffs with
 * stats == NULL provides them from the running statistics).
 * ------------------------------------------------------------------------- */
typedef struct mcamd_stem_block_desc {
    int32_t B, H, W;                      /* conv resolution; cin = 3 */
    const void* x;
    const void* wp;
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;   /* may be NULL */
    float momentum, eps;
    int32_t training;
    float* scale; float* shift; float* save_mean; float* save_invstd;   /* fp32 [32] each */
    float slope;                          /* 0.1 (leaky) or 1.0 (linear) */
    void* dst; int32_t dst_ld, dst_choff;
    /* backward only */
    const void* g; int32_t g_ld, g_choff;
    const float* mask;                    /* OIHW fp32 [32][3][3][3] or NULL */
    float grad_scale;
    float* dw;                            /* out: OIHW fp32, x mask, / grad_scale */
    float* dgamma; float* dbeta;          /* out fp32 [32], / grad_scale (may be NULL) */
    int32_t cout;                         /* filters: 32 (0 is read as 32); 8, 16 or 24 are accepted by the forward pass with
                                             training == 0 (physically slim models): `dst` still receives 32 channels, the
                                             ones past cout as zeros, and scale / shift hold cout entries */
    int32_t planes;                       /* forward: 1 (0 is read as 1), or 3 = split storage of the pooled output as in
                                             mcamd_act_desc.planes: hi | lo | hi in three ADJACENT 32-channel planes
                                             [dst_choff, dst_choff + 96) -- the "mixed" precision mode keeps plain fp16
                                             operands on this block (image and weights: 5.2e-4 -> 5.4e-4 on the logits,
                                             tools/error_budget.py) but hands its consumer an unrounded activation;
                                             2 = hi | lo in [dst_choff, dst_choff + 64) (consumer with x_wrap = 64) */
    /* SPLIT OPERANDS (round 4; both NULL = plain fp16 operands): the reference multiplies fp32 by fp32 (F.conv2d,
     * layers.py:60-64), and in TRAINING mode the operand rounding of this block alone moves the region-layer logits by
     * 1.9e-2.  With x_lo = fp16(x - fp16(x)) in a second NHWC4 image (mcamd_nchw_f32_to_nhwc4_split) and wp_lo =
     * fp16(w - fp16(w)) in the same packing as wp (mcamd_pack_stem_split) the pass accumulates
     * x_hi w_hi + x_lo w_hi + x_hi w_lo in fp32.  Honoured by mcamd_stem_block_stats and by mcamd_stem_block_fwd with
     * training == 0 (scale / shift read); the backward pass multiplies plain operands, as every backward pass does. */
    const void* x_lo;
    const void* wp_lo;
} mcamd_stem_block_desc;
size_t mcamd_stem_block_workspace_bytes(void);
/* dst == NULL with training != 0: the statistics half only -- Gram sums, scale / shift / save_mean / save_invstd and the
 * workspace context a later mcamd_stem_block_bwd reads; nothing is written to an output. */
int mcamd_stem_block_fwd(const mcamd_stem_block_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int mcamd_stem_block_bwd(const mcamd_stem_block_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Batch statistics of the block's conv output WITHOUT storing it (the training-mode forward on split operands is two
 * passes over the image: this one, mcamd_bn_coeffs on its slab, then mcamd_stem_block_fwd with training == 0):
 * stats[row][0][c] = sum over the pixels of workgroup `row` of y[.][c], stats[row][1][c] = sum of squares, fp32
 * [mcamd_stem_block_stats_rows(d)][2][stats_ld >= 32], every row written, fixed order (deterministic) -- the slab
 * mcamd_bn_coeffs takes, as mcamd_conv_epilogue.stats.  nn.BatchNorm2d's batch statistics (src/nets.py:802). */
int32_t mcamd_stem_block_stats_rows(const mcamd_stem_block_desc* d);
int mcamd_stem_block_stats(const mcamd_stem_block_desc* d, float* stats, int32_t stats_rows, int32_t stats_ld, void* stream);
/* How the block's five persistent launches divide a B x H x W problem (only d->B, H, W are read), from the function the
 * launches themselves ask; works without a GPU.  A work item is a unit (32 columns x 2 conv rows = 16 pooled pixels) or,
 * for the Gram pass, a step (32 columns x 1 row).  out[4 * launch + i], launch = MCAMD_STEM_PLAN_*:
 *   0 workgroups launched   1 work items   2 items all workgroups take in one pass (passes = ceil(items / this))
 *   3 items the busiest wave takes over all passes: the length of its fp32 accumulation chain
 * _FWD: the plain forward pass; _FWD_PLANES: the forward pass with planes >= 2 or split operands; _STATS:
 * mcamd_stem_block_stats (its grid is mcamd_stem_block_stats_rows); _GRAM: the Gram pass of training != 0; _BWD. */
#define MCAMD_STEM_PLAN_FWD 0
#define MCAMD_STEM_PLAN_FWD_PLANES 1
#define MCAMD_STEM_PLAN_STATS 2
#define MCAMD_STEM_PLAN_GRAM 3
#define MCAMD_STEM_PLAN_BWD 4
#define MCAMD_STEM_PLAN_LAUNCHES 5
#define MCAMD_STEM_PLAN_INFO_N 20
int mcamd_stem_block_plan_info(const mcamd_stem_block_desc* d, int32_t out[MCAMD_STEM_PLAN_INFO_N]);

/* ------------------------------------------------------------------------- *
 * Layout conversion at the model boundary (Darknet.forward takes/returns NCHW fp32,
 * nets.py:720-774).
 * ------------------------------------------------------------------------- */
/* src fp32 [B][C][H][W] * mul -> dst padded NHWC fp16 channels [choff, choff+C).  `overflow` (may be NULL): device
 * flag set to 1 when a value was clamped to +-65504 (the incoming logit gradient x grad_scale) -- and when the source
 * value is not finite: +-inf is stored as +-65504 and a NaN as -65504, finite gradients that must not pass for real ones. */
int mcamd_nchw_f32_to_padded_nhwc_f16(const float* src, int32_t B, int32_t C, int32_t H, int32_t W,
                                      float mul, void* dst, int32_t dst_ld, int32_t dst_choff, int32_t* overflow,
                                      void* stream);
/* As mcamd_nchw_f32_to_padded_nhwc_f16 with the destination in the shared-halo form when pad == 1. */
int mcamd_nchw_f32_to_padded_nhwc_f16_pad(const float* src, int32_t B, int32_t C, int32_t H, int32_t W,
                                          float mul, void* dst, int32_t dst_ld, int32_t dst_choff, int32_t pad,
                                          int32_t* overflow, void* stream);
/* The same into split storage (mcamd_act_desc.planes == 3): channel c of the image is written as hi = fp16(v) at
 * dst_choff + c, lo = fp16(v - hi) at dst_choff + plane + c and hi again at dst_choff + 2 * plane + c -- the network
 * input of the "fp16x3" / "mixed" precision modes (nets.py:720 takes the image as fp32 NCHW). */
int mcamd_nchw_f32_to_padded_nhwc_f16_split(const float* src, int32_t B, int32_t C, int32_t H, int32_t W,
                                            void* dst, int32_t dst_ld, int32_t dst_choff, int32_t plane, void* stream);

/* The image for the split-operand first block (mcamd_stem_block_desc.x / x_lo): src fp32 [B][3][H][W] -> two padded
 * NHWC4 fp16 images [B][H+2][W+2][4], hi = fp16(v) and lo = fp16(v - hi), channel 3 zero; the halo is not written
 * (zero it once).  nets.py:720 takes the image as fp32 NCHW. */
int mcamd_nchw_f32_to_nhwc4_split(const float* src, int32_t B, int32_t H, int32_t W, void* hi, void* lo, void* stream);
/* The stem packing of mcamd_pack_weights (g->stem) for split operands: wp_hi = fp16(w * mask), wp_lo =
 * fp16(w * mask - wp_hi), both [Npad][96]. */
int mcamd_pack_stem_split(const float* w_oihw, const float* mask_oihw, int32_t cout, void* wp_hi, void* wp_lo, void* stream);

/* The first convolution of the split-operand precisions in fp32 on the vector ALUs, straight from the image
 * (F.conv2d(x, weight * mask, None, 1, 1) at layers.py:60-64 for a 3-channel input, 3x3 kernel, 32 filters):
 *   x_nchw fp32 [B][3][H][W] -> y fp32 [B*H*W][y_ld] (channels 0..31), exact fp32 products and sums;
 *   stats (may be NULL): fp32 [stats_rows][2][stats_ld] partial sums / sums of squares of y per filter, one row per
 *   workgroup, stats_rows == mcamd_stem_conv_f32_stats_rows(); mcamd_bn_coeffs adds the rows (training mode);
 *   weff_scratch: 32 * 27 floats of device memory the call may overwrite (weight * mask).
 * Other filter counts are refused (the caller then multiplies split operands through mcamd_conv_fwd). */
int32_t mcamd_stem_conv_f32_stats_rows(void);
int mcamd_stem_conv_f32(const float* x_nchw, int32_t B, int32_t H, int32_t W, const float* w_oihw,
                        const float* mask_oihw, int32_t cout, float* weff_scratch, float* y, int32_t y_ld,
                        float* stats, int32_t stats_rows, int32_t stats_ld, void* stream);

/* ------------------------------------------------------------------------- *
 * Region loss of the training step (reference src/nets.py:282-635: build_targets + RegionLoss.forward, called at
 * train.py:224): loss AND d(loss)/d(output) in one pass over the logits; the targets are built per image in LDS.
 *   output : fp32 [B][num_anchors * (5 + num_classes)][H][W] -- what Darknet.forward returns (nets.py:720-774)
 *   target : fp32 [B][max_boxes * 5] rows of (class, x, y, w, h), normalised to [0, 1]; a row list ends at the first x == 0
 *   anchors: num_anchors (w, h) pairs in grid units (the [region] block of the cfg)
 *   loss   : device fp32 scalar = the value RegionLoss.forward returns (sum of the six terms / B)
 *   grad   : device fp32, shaped like output: d(loss)/d(output)
 *   counts : optional device int32[2] (nGT, nCorrect; the reference prints them), ADDED to -- zero them first
 * The reference's arithmetic quirks are kept (modelcompression_amd/region_loss.py lists them).  Deterministic.
 * ------------------------------------------------------------------------- */
typedef struct mcamd_region_desc {
    const float* output; const float* target;
    int32_t B, H, W, num_anchors, num_classes, max_boxes;   /* max_boxes must be 50 (nets.py:312) */
    float anchors[16];
    float coord_scale, noobject_scale, object_scale, class_scale, thresh;
} mcamd_region_desc;
size_t mcamd_region_loss_workspace_bytes(int32_t B);
int mcamd_region_loss(const mcamd_region_desc* d, float* loss, float* grad, int32_t* counts, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Objectness-scaled distillation loss of a YOLOv2 head against a frozen teacher's logits (Mehta and Ozturk, "Object
 * detection at 200 FPS"; Chen et al., NeurIPS 2017): loss AND d(loss)/d(student) in one pass, no gradient for the teacher.
 *   student, teacher : fp32 [B][num_anchors * (5 + num_classes)][H][W] -- what Darknet.forward returns; per prediction
 *                      (x, y, w, h, obj, classes) with student values s_k and teacher values t_k:
 *     q   = sig(t_4)                                        (a weight, never differentiated)
 *     L_o = 1/2 (sig(s_4) - q)^2
 *     L_b = 1/2 [(sig(s_0) - sig(t_0))^2 + (sig(s_1) - sig(t_1))^2 + (s_2 - t_2)^2 + (s_3 - t_3)^2]
 *     L_c = temperature^2 * KL(softmax(t_5.. / temperature) || softmax(s_5.. / temperature))
 *     loss = 1/B sum [obj_scale L_o + q (box_scale L_b + cls_scale L_c)]
 *   loss : device fp32 scalar;  grad : device fp32, shaped like student: d(loss)/d(student)
 *   workspace : mcamd_distill_loss_workspace_bytes(B, num_anchors) bytes, one partial sum per (image, anchor)
 * Deterministic (no atomics); bit-equal operands give loss == 0 and grad == 0 exactly; a NaN or Inf logit in either
 * operand gives a non-finite loss.  num_anchors in [1, 8], num_classes >= 1, temperature > 0.
 * ------------------------------------------------------------------------- */
typedef struct mcamd_distill_desc {
    const float* student; const float* teacher;
    int32_t B, H, W, num_anchors, num_classes;
    float obj_scale, box_scale, cls_scale, temperature;
} mcamd_distill_desc;
size_t mcamd_distill_loss_workspace_bytes(int32_t B, int32_t num_anchors);
int mcamd_distill_loss(const mcamd_distill_desc* d, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------- *
 * Detection post-processing of the eval path (reference src/nets2_utils.py:141-259 get_region_boxes + nms, chained as
 * predict.py:148-173 does).  N = H * W * num_anchors rows per image in the reference's (cy, cx, anchor) order,
 * N <= 2048, num_anchors <= 8, num_classes <= 80; anything else returns MCAMD_EINVAL and launches nothing.
 * None of the three allocates, synchronises or can be recorded into a launch plan.
 *   output  : fp32 [B][num_anchors * (5 + num_classes)][H][W] -- what Darknet.forward returns
 *   anchors : num_anchors (w, h) pairs in grid units
 *
 * mcamd_region_decode: head [B][N][7] = x, y, w, h (network-relative), box_conf, cls_max_conf, cls_max_id (as float;
 *   the first maximum), cls_conf [B][N][num_classes] = the softmax class confidences.
 *
 * mcamd_nms: greedy suppression of nets2_utils.py:236-259 for B images of n <= 2048 boxes (cx, cy, w, h), 16-byte
 *   aligned.  order [B][n]: the stable ascending sort of the fp32 key 1.0f - conf (ties by lower index) over all n
 *   entries; kept [B][n]: whether the r-th box of that order survives.  Candidates are conf > 0; a candidate is kept iff
 *   no KEPT box before it in the order has iou > nms_thresh with it (bbox_iou, x1y1x2y2=False, strict).
 *
 * mcamd_detect: decode, candidates box_conf * cls_max_conf > conf_thresh, sort by 1 - box_conf, suppression and
 *   compaction in one launch.  rows [B][N][8]: the kept boxes by descending confidence, the seven head values and the
 *   row index n (as float); probs [B][N][num_classes] = box_conf * cls_conf of the same rows; nkept [B] = kept boxes per
 *   image.  Rows at or beyond nkept[b] are unspecified.  head_out / cls_out (each may be NULL) receive the full decode,
 *   bit-equal to mcamd_region_decode's.
 * ------------------------------------------------------------------------- */
typedef struct mcamd_detect_desc {
    const float* output;
    int32_t B, H, W, num_anchors, num_classes;
    float anchors[16];
    float conf_thresh, nms_thresh;                            /* mcamd_detect only */
} mcamd_detect_desc;
int mcamd_region_decode(const mcamd_detect_desc* d, float* head, float* cls_conf, void* stream);
int mcamd_nms(const float* boxes, const float* conf, int32_t B, int32_t n, float nms_thresh, int32_t* order,
              uint8_t* kept, void* stream);
int mcamd_detect(const mcamd_detect_desc* d, float* rows, float* probs, int32_t* nkept, float* head_out,
                 float* cls_out, void* stream);

/* ------------------------------------------------------------------------- *
 * VOC07 evaluation on the device (reference src/predict.py:250-437, voc_eval + voc_ap with use_07_metric=True), fed by
 * what mcamd_detect writes.  The per-class AP values are the float64 values that the reference's file path computes
 * from the same detections: it prints every fp32 score and coordinate with "%f" and parses the text as a double, which
 * is q(v) = rint((double)v * 1e6) / 1e6 exactly.  Neither call allocates, synchronises or can be recorded into a launch
 * plan; every limit is checked before the launch (MCAMD_EINVAL, nothing launched).
 *
 * mcamd_voc_match: for image b of the batch, row r < nkept[b] and class c, a record is emitted when
 *   probs[b][r][c] > conf_thresh or c == cls_max_id of the row (rows[b][r][6]); rows at or beyond nkept[b] are never
 *   read.  Its box is x1 = q(fl32(fl32(x - fl32(w / 2)) * W)), y1, x2 (+), y2 likewise with the image's (W, H) as fp32.
 *   Per (image, class) the records are matched in the order (descending q(score), ascending r) against the image's
 *   ground-truth objects of that class in table order, in float64 term by term as voc_eval writes it:
 *   iw = max((min(g2, b2) - max(g0, b0)) + 1., 0.), ih likewise, uni = ((b2 - b0 + 1.) * (b3 - b1 + 1.) +
 *   (g2 - g0 + 1.) * (g3 - g1 + 1.)) - iw * ih; the first maximum of iw * ih / uni wins; with no object of the class the
 *   maximum is -inf.  flag = 1 (tp) when the maximum > ovthresh and its object is neither difficult nor matched yet (it
 *   is matched from then on), 0 (neither) when that object is difficult, 2 (fp) otherwise.
 *   Every record takes a slot from counters[0] (atomically; slot order is arbitrary) and writes keys[slot], flags[slot];
 *   a record whose slot is >= capacity is counted in counters[1] and not written.  The caller zeroes counters before the
 *   first batch.  The 64-bit key is a total order, class, then descending q(score), then image, then row:
 *       bit 63      0 (the keys also sort as signed 64-bit integers)
 *       bits 62-56  class
 *       bits 55-36  1000000 - rint(score * 1e6)
 *       bits 35-11  first_image + b              (first_image + B <= 2^25)
 *       bits 10-0   r
 *   Limits: N <= 2048, C <= 80, G <= 64.
 *     rows, probs, nkept : [B][N][8], [B][N][C], [B] as mcamd_detect writes them
 *     gt_box             : int32 [B][G][4] xmin, ymin, xmax, ymax;  gt_cls, gt_difficult: uint8 [B][G];
 *     gt_count           : int32 [B] objects per image (<= G);  image_size: int32 [B][2] width, height
 *
 * mcamd_voc_ap: keys / flags are the records SORTED by key (flags permuted alike), n = min(counters[0], capacity) of
 *   them; npos [C] = non-difficult objects per class.  Per class, over its records in order:
 *   rec = tp_cum / (double)max(npos, 1), prec = tp_cum / max(tp_cum + fp_cum, DBL_EPSILON), p_i = the maximum of prec
 *   where rec >= i * 0.1 (0 when nowhere), ap = the sequential sum of p_i / 11., i = 0 .. 10; 0.0 without records.
 *   ap [C]; rec, prec (each may be NULL) receive the curves at the records' sorted positions.
 * ------------------------------------------------------------------------- */
typedef struct mcamd_voc_match_desc {
    const float* rows; const float* probs; const int32_t* nkept;
    int32_t B, N, C, G;
    float conf_thresh;
    int32_t first_image;
    double ovthresh;
    const int32_t* gt_box; const uint8_t* gt_cls; const uint8_t* gt_difficult; const int32_t* gt_count;
    const int32_t* image_size;
    uint64_t* keys; uint8_t* flags; int64_t capacity;
    uint64_t* counters;                                       /* [0] records, [1] records lost to the capacity */
} mcamd_voc_match_desc;
int mcamd_voc_match(const mcamd_voc_match_desc* d, void* stream);
int mcamd_voc_ap(const uint64_t* keys, const uint8_t* flags, const uint64_t* counters, int64_t capacity,
                 const int32_t* npos, int32_t C, double* ap, double* rec, double* prec, void* stream);

/* ------------------------------------------------------------------------- *
 * Training augmentation (reference src/dataloader.py:148-178 data_augmentation + ToTensor(), train=True): per image
 * crop (outside the source reads 0) -> Pillow bicubic resize -> optional left-right flip -> Pillow RGB->HSV, three
 * point LUTs, HSV->RGB -> out = u8 / 255.f.  Bit-equal to the reference's PIL chain: the host builds Pillow's
 * fixed-point tables and the LUTs (modelcompression_amd/augment.py), the device only applies them.  Two launches
 * (horizontal pass into tmp, then vertical pass + flip + HSV + store); no host synchronisation.
 *   src  : uint8 RGB sources, HWC, rows of src_w * 3 bytes, image b at src + desc[b].src_off
 *   coef : int32 resampling tables; a table for n outputs with k taps is n rows of (first, count, k[0..k-1]):
 *          output o = clip8((2^21 + sum_t in[first + t] * k[t]) >> 22), t < count
 *   lut  : uint8 [3][256] per image (H, S, V) at lut + desc[b].lut_off
 *   tmp  : workspace (4-byte aligned), crop_h rows of W * 4 bytes (R, G, B, 0) per image at tmp + desc[b].tmp_off
 *   out  : fp32 [B][3][H][W]
 * A descriptor with lut_off == -1 has no HSV step: out = u8 / 255.f of the resampled pixel (Image.resize +
 * ToTensor()); lut may be NULL when no image has LUTs.  Every other negative lut_off is refused.
 * Returns MCAMD_EINVAL for an empty crop (crop_w or crop_h < 1: the reference makes an image of no pixels there) and
 * for any table / LUT / source / workspace extent outside its buffer; nothing is launched then.
 * ------------------------------------------------------------------------- */
typedef struct mcamd_augment_desc {
    int64_t src_off;            /* byte offset of the source in src */
    int64_t tmp_off;            /* byte offset of this image's horizontal-pass rows in tmp, a multiple of 4 */
    int32_t src_w, src_h;       /* source size, pixels */
    int32_t crop_x, crop_y;     /* crop origin in source pixels (pleft, ptop; may be negative) */
    int32_t crop_w, crop_h;     /* crop size (swidth - 1, sheight - 1: the reference's box is inclusive-exclusive) */
    int32_t flip;               /* left-right flip after the resize */
    int32_t hk, vk;             /* taps per row of the horizontal (W rows) and vertical (H rows) tables */
    int32_t hcoef_off, vcoef_off; /* int32 offsets of the two tables in coef */
    int32_t lut_off;            /* byte offset of the [3][256] LUTs in lut; -1: no HSV distortion */
} mcamd_augment_desc;
typedef struct mcamd_augment_batch {
    const mcamd_augment_desc* desc;      /* HOST array of B descriptors: validated */
    const mcamd_augment_desc* desc_dev;  /* the same B descriptors in device memory: what the kernels read */
    const uint8_t* src; int64_t src_bytes;
    const int32_t* coef; int64_t coef_elems;
    const uint8_t* lut; int64_t lut_bytes;
    uint8_t* tmp; int64_t tmp_bytes;
    float* out;
    int32_t B, H, W;
} mcamd_augment_batch;
int mcamd_augment(const mcamd_augment_batch* a, void* stream);
/* The tables and LUTs of a batch built on the device, for sources that already live there: for every image the
 * horizontal table (crop_w -> W) at coef + hcoef_off, the vertical table (crop_h -> H) at coef + vcoef_off and, when
 * lut_off >= 0, the LUTs of hsv_dev[b] = (dhue, dsat, dexp) at lut + lut_off.  The contract is augment.resample_table
 * and augment.point_luts (modelcompression_amd/augment.py) bit for bit, in the row format above: float64 throughout,
 * the same operations in the same order, the row sum in tap order, truncation toward zero, round-half-even for the
 * LUTs, the hue wrap at 255, the identity table (k = 1) where the sizes are equal.  One launch, no host
 * synchronisation; mcamd_augment on the same stream then reads what this wrote.
 *   desc_host / desc_dev : the B descriptors of mcamd_augment_batch (host copy validated, device copy read)
 *   hsv_dev              : float64 [B][3] in device memory; may be NULL when every lut_off is -1 (lut too)
 * Returns MCAMD_EINVAL, before anything is launched, when a table or LUT extent lies outside its buffer, when hk or vk
 * is not the tap count of its table (1 for equal sizes, else 2 * ceil(2 * max(float(n_in) / n_out, 1)) + 1), or when a
 * crop is empty. */
int mcamd_augment_tables(const mcamd_augment_desc* desc_host, const mcamd_augment_desc* desc_dev, const double* hsv_dev,
                         int32_t B, int32_t H, int32_t W, int32_t* coef, int64_t coef_elems, uint8_t* lut,
                         int64_t lut_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Launch plans: a whole forward or backward pass as ONE library call.
 * The reference executes Darknet.forward as one Python call per torch module (src/nets.py:720-774) and autograd
 * replays them; here the caller walks its layer list ONCE between mcamd_plan_begin and mcamd_plan_end: every
 * launch-type entry point above (pack / fold / conv fwd / dgrad / wgrad / bn_coeffs / bn_act fwd + bwd / stem block /
 * layout conversion / mcamd_stream_wait / mcamd_memset_zero) then RECORDS its arguments -- descriptors copied by
 * value -- instead of launching, on the recording host thread only.  mcamd_plan_run replays them: same launches, same
 * order, same streams (bit-identical results), without the per-launch host overhead of a language binding.
 * A plan holds the raw device pointers it was recorded with: the caller keeps those buffers in place and records a
 * new plan when one moves.  Argument errors of a recorded call surface from mcamd_plan_run.  Queries
 * (*_workspace_bytes, tile_info, ...) are never recorded.
 *   streams  : the hipStream_t's (as void*) the recording may see, slot 0 first; mcamd_plan_run takes the streams to
 *              replay on in the same slot order (normally the same ones)
 *   segments : mcamd_plan_mark() closes a segment; mcamd_plan_run(p, lo, hi, ...) replays segments [lo, hi) -- the
 *              data-parallel reducer is called between segments, when a gradient slice has become final
 * ------------------------------------------------------------------------- */
typedef struct mcamd_plan mcamd_plan;
int mcamd_plan_begin(void* const* streams, int32_t nstreams);
int32_t mcamd_plan_mark(void);                    /* -> index of the segment that starts here */
mcamd_plan* mcamd_plan_end(void);                 /* NULL when a recorded call failed (mcamd_last_error) */
int32_t mcamd_plan_segments(const mcamd_plan* p);
int32_t mcamd_plan_launches(const mcamd_plan* p); /* recorded calls (a call may launch several kernels) */
int mcamd_plan_run(mcamd_plan* p, int32_t seg_lo, int32_t seg_hi, void* const* streams, int32_t nstreams);
void mcamd_plan_destroy(mcamd_plan* p);
/* `waiter` waits for all work enqueued so far on `signal` (event record + stream wait; the two-stream backward pass
 * hands weight gradients to its second stream this way).  Recordable. */
int mcamd_stream_wait(void* waiter_stream, void* signal_stream);
/* hipMemsetAsync(dst, 0, bytes) -- the zero rows of a filter-pruned layer's weight gradient.  Recordable. */
int mcamd_memset_zero(void* dst, size_t bytes, void* stream);

/* The overflow / non-finite policy of a training step as ONE launch (modelcompression_amd/train.py StepGuard; the
 * reference checks the loss on the host, train.py:226-231):
 *   flags[0] = any of the n_engine device flags engine_overflow[i] (mcamd_conv_epilogue.overflow & co.) is set,
 *   flags[1] = *loss is not finite (loss may be NULL), flags[2] = *transport_overflow != 0 (may be NULL);
 *   the int flags that were read are reset to 0; found (may be NULL) = flags[0] + flags[1] + flags[2] -- what torch's
 *   fused SGD takes as `found_inf`.
 * With n_engine == 0, loss == NULL and transport_overflow == NULL only `found` is recomputed from `flags` (after the
 * MAX all-reduce of the flags over the data-parallel ranks).  engine_overflow: host array of <= 8 device pointers. */
int mcamd_step_flags(const int32_t* const* engine_overflow, int32_t n_engine, const float* loss,
                     int32_t* transport_overflow, float* flags, float* found, void* stream);

/* ------------------------------------------------------------------------- *
 * Pruning (reference src/pruning/weightPruning/methods.py).
 * ------------------------------------------------------------------------- */
/* k-th smallest |w| (0-based, ascending) over `nseg` fp32 tensors -- the order statistic
 * np.percentile selects at methods.py:18.  Writes s[k] and s[min(k+1, n-1)] as two fp32 values to
 * `out2` (device).  ptrs/counts are HOST arrays of device pointers / element counts. */
size_t mcamd_kth_magnitude_workspace_bytes(void);
int mcamd_kth_magnitude(const float* const* ptrs, const int64_t* counts, int32_t nseg, int64_t k,
                        float* out2, void* workspace, size_t workspace_bytes, void* stream);
/* mask[i] = |w[i]| > *threshold ? 1.f : 0.f  (strict, methods.py:24-25); threshold is a device fp32. */
int mcamd_magnitude_mask(const float* w, int64_t n, const float* threshold, float* mask, void* stream);
/* Per-filter score of methods.py:43-51 in numpy's fp32 summation order:
 * out[o] = (mean_sq[o] / sqrt(sum_o mean_sq^2)) / max_o(...), one launch per conv layer. */
size_t mcamd_filter_scores_workspace_bytes(int32_t cout);
int mcamd_filter_scores(const float* w_oihw, int32_t cout, int32_t cin, int32_t kh, int32_t kw,
                        float* scores, void* workspace, size_t workspace_bytes, void* stream);
/* Only the first stage: out[o] = sum(w[o]^2) / (cin*kh*kw) in numpy's summation order
 * (prune_one_filter ranks before the /max step, methods.py:104-109).  Same workspace size. */
int mcamd_filter_mean_square(const float* w_oihw, int32_t cout, int32_t cin, int32_t kh, int32_t kw,
                             float* mean_sq, void* workspace, size_t workspace_bytes, void* stream);
/* mask[o][...] = keep[o] ? 1.f : 0.f over a [cout][per_filter] tensor (methods.py:74). */
int mcamd_filter_mask(const int32_t* keep, int32_t cout, int64_t per_filter, float* mask, void* stream);
/* count of exact zeros in an fp32 tensor, added to *out (device int64) -- prune_rate, utils.py:76-80. */
int mcamd_count_zeros(const float* w, int64_t n, unsigned long long* out, void* stream);
/* sum(p * |m - 1|) accumulated in fp32 into *out -- are_masks_consistent, utils.py:122-133. */
int mcamd_masked_residual(const float* w, const float* mask, int64_t n, float* out, void* stream);

/* N:M magnitude mask (nm_prune, an addition beyond the reference) of an OIHW tensor [cout][cin][khw], cin % 4 == 0:
 * in every group of 4 consecutive input channels at a fixed (filter, tap) the 2 entries with the largest
 * |w * old_mask| keep their old mask value (1 when old_mask is NULL), the others get 0; ties keep the lower channel.
 * n = 2, m = 4 only. */
int mcamd_nm_mask(const float* w, const float* old_mask, int32_t cout, int32_t cin, int32_t khw, int32_t n, int32_t m,
                  float* mask, void* stream);
/* number of such groups holding more than 2 non-zero mask entries, added to *count (device int32) */
int mcamd_nm_violations(const float* mask, int32_t cout, int32_t cin, int32_t khw, int32_t* count, void* stream);

/* Block magnitude scores (block_prune, an addition beyond the reference) of an OIHW tensor [cout][cin][khw], cin % 32 == 0.
 * Block (fb, cb, tap): filters [64 fb, min(64 fb + 64, cout)) x input channels [kb cb, kb cb + kb) at one tap, kb = 64 when
 * cin % 64 == 0 else 32 -- one K chunk of one N tile of mcamd_conv_fwd_bsparse; block index (fb * (cin / kb) + cb) * khw + tap.
 * scores[block] = the float64 mean over the block of (double)(w * old_mask)^2 (old_mask may be NULL = ones; the product
 * in fp32).  Fixed summation order, no atomics: with the block's elements numbered e = r * kb + c, lane l of one wave adds
 * e = l, l + 64, ... in ascending order; the 64 lane sums are combined by s[l] += s[l ^ d], d = 32, 16, 8, 4, 2, 1. */
int mcamd_block_scores(const float* w, const float* old_mask, int32_t cout, int32_t cin, int32_t khw, double* scores,
                       void* stream);
/* mask = old_mask (NULL = ones) with every block whose keep[block index] is 0 zeroed. */
int mcamd_block_mask(const int32_t* keep, const float* old_mask, int32_t cout, int32_t cin, int32_t khw, float* mask,
                     void* stream);

/* ------------------------------------------------------------------------- *
 * Compressed model files (.mcz; an addition beyond the reference): the two device passes around the file.
 * ------------------------------------------------------------------------- */
/* The file (little-endian, every array zero-padded to a multiple of 8 bytes):
 *   header   char magic[4] = "MCZW"; uint32 version = 1; uint32 payload (value kind the file was asked for);
 *            uint32 nrec; int64 seen
 *   record   int32 cout, cin, kh, kw; uint32 flags; uint32 0; uint64 kept;
 *            float32 bn.bias[cout], bn.weight[cout], running_mean[cout], running_var[cout]   (MCAMD_WZ_F_BN)
 *            or float32 conv.bias[cout];
 *            int32 exponent[cout]                                                            (value kind MCAMD_WZ_FP8)
 *            uint64 word[ceil(n / 64)], n = cout cin kh kw                                   (MCAMD_WZ_F_BITS)
 *            kept values (MCAMD_WZ_F_BITS) or all n values, in flat OIHW order
 *   flags    MCAMD_WZ_F_BN | MCAMD_WZ_F_BITS | value kind << 8
 * Bit i of word j stands for weight 64 j + i; the tail bits of the last word are 0.  A weight is KEPT iff its stored
 * value is non-zero: any bit outside the sign bit set in the code of weight * mask, the code being
 *   MCAMD_WZ_FP32  the fp32 pattern,            4 bytes
 *   MCAMD_WZ_FP16  its round-to-nearest-even fp16 pattern (what the fp16 packers store),   2 bytes
 *   MCAMD_WZ_FP8   the e4m3 code mcamd_pack_q8 stores, with that packer's exponent per filter,   1 byte
 * and every other weight reads back as +0.  A record has bit words iff 8 ceil(n / 64) + kept elem < n elem; otherwise
 * all n values are stored (0 for a weight that is not kept).  Reading: fp32 as is, fp16 widened, e4m3 as
 * value(code) 2^-exponent (exact in fp32 whenever that is a normal number).
 *
 * A fourth kind stores a layer tied by weight sharing (below):
 *   MCAMD_WZ_CODE  the codebook index of the weight, 1 byte in the passes, `width` bits in the file
 * A weight of this kind is KEPT iff its MASK value is non-zero (every weight when there is no mask): a shared value may
 * be exactly 0, so the bits cannot come from the values.  Its record carries `bits` (1..8) in the uint32 behind the flags
 * (0 for the other kinds) and, behind the per-channel arrays, float32 codebook[2^bits]; then the bit words, then the codes
 * of the kept weights (or of all n, 0 where not kept) in flat order, `width` bits each, code i in bits
 * [width (i % (8 / width)), +width) of byte i / (8 / width), width = the smallest of 1, 2, 4, 8 that is >= bits.  It has
 * bit words iff kept < n (a code cannot say "not kept", so the size rule of the other kinds does not apply).  The passes
 * see one byte per code: pack reads w = uint8 codes[n] and stores the kept ones by the same rule; unpack writes
 * w = uint8 codes[n] (0 where the bit is clear) and the mask.  A file whose header payload is MCAMD_WZ_CODE stores its
 * untied layers as MCAMD_WZ_FP32.
 *
 * A fifth kind stores a layer as the 4-bit engine consumes it (mcamd_pack_q8_w4 above), cin % 32 == 0:
 *   MCAMD_WZ_W4    the 4-bit code of the weight (bit 3 sign, bits 0-2 grid index, never -0), 1 byte in the passes, one
 *                  nibble in the file
 * Behind the per-channel arrays its record carries int32 e4[cout], the filter exponents of mcamd_pack_q8_w4, and
 * uint8 shift[n / 32], g + 5 (0..11) of every group of 32 input channels at one tap in the order [cout][cin / 32][kh][kw]
 * (an all-zero group: byte 0); then the bit words, then the codes of the kept weights (or of all n, 0 where not kept) in
 * flat OIHW order, code i in bits [4 (i % 2), +4) of byte i / 2, the unused nibble of the last byte 0.  Codes, shifts and
 * exponents are exactly those of mcamd_pack_q8_w4 on the same weight * mask, in OIHW order instead of the kernel's tile
 * layout.  A weight is KEPT iff code & 7 != 0; the record has bit words iff
 * 8 ceil(n / 64) + ceil(kept / 2) < ceil(n / 2).  Reading: grid[code & 7] 2^(shift - 5 - e4) with the code's sign (exact
 * in fp32 whenever that is a normal number); a shift byte above 11 reads as +0.  A file whose header payload is
 * MCAMD_WZ_W4 stores its other layers as MCAMD_WZ_FP16.  The passes see one byte per code, as for MCAMD_WZ_CODE, through
 * mcamd_wz_pack_w4 / mcamd_wz_unpack_w4 (below), which take the shift bytes as one more array. */
#define MCAMD_WZ_FP32 0
#define MCAMD_WZ_FP16 1
#define MCAMD_WZ_FP8 2
#define MCAMD_WZ_CODE 4 /* (3 is not a kind) */
#define MCAMD_WZ_W4 5
/* mcamd_wz_seg.kind of an MCAMD_WZ_W4 segment also carries the taps kh kw of its tensor (a group of 32 input channels is
 * strided by them in OIHW); every other kind is the bare value */
#define MCAMD_WZ_W4_KIND(taps) (MCAMD_WZ_W4 | (taps) << 8)
#define MCAMD_WZ_F_BN 1u
#define MCAMD_WZ_F_BITS 2u
#define MCAMD_WZ_BLOCK_WORDS 64 /* bit words (of 64 weights) per workgroup of both passes */

/* One weight tensor of a pass.  All tensors of a model go through ONE table: a HOST array for the checks and the grid
 * sizes and its DEVICE copy for the kernels.  Running sums over the table, in order (checked):
 *   block0  += ceil(ceil(n / 64) / MCAMD_WZ_BLOCK_WORDS)
 *   word0   += ceil(n / 64)     pack only
 *   exp0    += cout             pack only, the segments of kind MCAMD_WZ_FP8 and MCAMD_WZ_W4
 *   shift0  += ceil(n / 256)    pack only, the segments of kind MCAMD_WZ_W4 (its n / 32 shift bytes, padded to 8)
 * Unpack reads the bit words, exponents, shift bytes and values where the caller has them: word0 (dense == 0), exp0
 * (MCAMD_WZ_FP8, MCAMD_WZ_W4), shift0 (MCAMD_WZ_W4) and val0 are any offsets whose range lies inside the arrays given
 * (checked).  All the arrays may be one buffer holding the file as it is, since every array of a record starts at a
 * multiple of 8 bytes. */
typedef struct mcamd_wz_seg {
    void* w;         /* fp32 OIHW [cout][n / cout]: the master (pack, read) or the weights to fill (unpack, written);
                        MCAMD_WZ_CODE: uint8 codes [n] */
    void* mask;      /* fp32 0/1 mask: read by pack (NULL = all ones); written by unpack unless NULL */
    int64_t n;       /* weights, > 0, a multiple of cout */
    int64_t word0;   /* first bit word of the segment in `words` */
    int64_t val0;    /* unpack: byte offset of the segment's values in `values`, a multiple of 8.  pack: unused */
    int64_t kept;    /* unpack, dense == 0: number of values stored (<= n).  pack: unused */
    int32_t cout;
    int32_t kind;    /* MCAMD_WZ_FP32 / _FP16 / _FP8 / _CODE, or MCAMD_WZ_W4_KIND(kh kw) */
    int32_t exp0;    /* first exponent of the segment in `exps` */
    int32_t dense;   /* unpack: 1 = the record has no bit words, all n values are stored.  pack: unused */
    int32_t block0;  /* first workgroup of the segment */
    int32_t shift0;  /* MCAMD_WZ_W4: first shift byte of the segment in `shifts`, in units of 8 bytes.  Otherwise unused */
} mcamd_wz_seg;

/* workspace of either pass for a table of `nseg` segments and `nblocks` workgroups (the final block0 sum) */
size_t mcamd_wz_workspace_bytes(int64_t nblocks, int32_t nseg);

/* Pack: for every segment the bit words (words[word0 ...]), the kept count (counts[segment], uint64), the exponents of an
 * MCAMD_WZ_FP8 segment (exps[exp0 ...]) and the values.  The values of segment s begin at byte
 *   base(s) = sum over t < s of round_up(bytes(t), 8),  bytes(t) = (record t has bit words ? kept : n) * elem
 * of `values`, by the rule above -- exactly the value arrays of the file, padding included (the padding bytes are not
 * written: zero `values` first).  values_bytes >= sum of round_up(n elem, 8) (checked).  One wave per word: the ballot of
 * "my weight is kept" IS the word, a lane's rank is the population count of the word below the lane; positions come
 * from a scan of the per-workgroup counts -- no atomics, the output bytes depend on the inputs only.
 * Not recordable into a launch plan (refused while a recording is open). */
int mcamd_wz_pack(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, uint64_t* words, int64_t words_cap,
                  uint64_t* counts, int32_t* exps, int64_t exps_cap, void* values, int64_t values_bytes, void* workspace,
                  size_t workspace_bytes, void* stream);

/* Unpack: the reverse, next to the weights: w[i] = the value bit i selects (+0 where the bit is clear), mask[i] = the bit
 * as 0.f / 1.f (all ones for a dense segment).  A bit whose position is past `kept` reads as +0 (a damaged file cannot
 * make the pass read outside `values`; val0 + stored bytes <= values_bytes is checked).  Not recordable. */
int mcamd_wz_unpack(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, const uint64_t* words,
                    int64_t words_cap, const int32_t* exps, int64_t exps_cap, const void* values, int64_t values_bytes,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The two passes for a table that may hold MCAMD_WZ_W4 segments (any other kind as above, and a table without one gives
 * the bytes of mcamd_wz_pack / mcamd_wz_unpack).  `shifts` holds the shift bytes, segment s at byte 8 shift0.
 * Pack: a pre-pass (one workgroup per filter) takes the filter maximum and from it e4_f (exps[exp0 ...]), then the maxima
 * of the filter's groups and from them the shift bytes; in the word and scatter passes each lane derives its own code from
 * its weight, its filter's e4_f and its group's shift by the rule of mcamd_pack_q8_w4 (csrc/w4_quant.h, one statement for
 * both).  The values of an MCAMD_WZ_W4 segment are one byte per code, bytes(t) = (bit words ? kept : n), bit words iff
 * 8 ceil(n / 64) + ceil(kept / 2) < ceil(n / 2); the caller packs two codes into a byte for the file.  shifts_cap >= the
 * final shift0 sum * 8 (checked); the padding bytes are not written: zero `shifts` first.
 * Unpack: w[i] = grid[code & 7] 2^(shift - 5 - e4_f) with the code's sign and the mask as above, from one byte per code at
 * val0 (the caller widens the file's nibbles).  A shift byte above 11 and a code position past `kept` read as +0; every
 * offset is checked against the capacities given before the launch. */
int mcamd_wz_pack_w4(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, uint64_t* words, int64_t words_cap,
                     uint64_t* counts, int32_t* exps, int64_t exps_cap, void* values, int64_t values_bytes, void* workspace,
                     size_t workspace_bytes, void* stream, uint8_t* shifts, int64_t shifts_cap);
int mcamd_wz_unpack_w4(const mcamd_wz_seg* segs, const mcamd_wz_seg* segs_dev, int32_t nseg, const uint64_t* words,
                       int64_t words_cap, const int32_t* exps, int64_t exps_cap, const void* values, int64_t values_bytes,
                       void* workspace, size_t workspace_bytes, void* stream, const uint8_t* shifts, int64_t shifts_cap);

/* ------------------------------------------------------------------------- *
 * Huffman-coded model files ("MCZH"; an addition beyond the reference): the device passes around the file.
 * ------------------------------------------------------------------------- */
/* The coded file is the "MCZW" file above with every uint8-symbol array replaced by a STREAM; it is a container of its own:
 *   header   char magic[4] = "MCZH"; uint32 version = 1; then payload, nrec, seen as above
 *   record   the 32-byte record header, the per-channel float arrays, the int32 exponents and the fp32 codebook byte for
 *            byte as above (same flags, `bits`, `kept`, same rule for bit words); in the place of
 *              the shift bytes (MCAMD_WZ_W4)     a stream of the n / 32 bytes,                        alphabet A = 12
 *              the bit words (MCAMD_WZ_F_BITS)   a stream of the 8 ceil(n / 64) bytes of the words,   A = 256
 *              the values, MCAMD_WZ_FP8          a stream of the stored e4m3 bytes,                   A = 256
 *              the values, MCAMD_WZ_CODE         a stream of one symbol per stored code,              A = 2^bits
 *              the values, MCAMD_WZ_W4           a stream of one symbol per stored nibble code,       A = 16
 *            MCAMD_WZ_FP16 and MCAMD_WZ_FP32 values stay the raw arrays of the "MCZW" file.
 *   stream   uint32 mode (0 raw, 1 Huffman); uint32 A; uint64 nsym; then
 *     mode 0   the array exactly as the "MCZW" file stores it (codes packed at their width), padded to 8 bytes
 *     mode 1   uint64 nbits
 *              uint8  length[A]                                 0 = symbol absent, else 1..MCAMD_HZ_MAXLEN; padded to 8 bytes
 *              uint32 chunk_bit0[ceil(nsym / MCAMD_HZ_CHUNK)]   bit position of each chunk's first code; padded to 8 bytes
 *              uint64 bits[ceil(nbits / 64)]
 * Codes are canonical (RFC 1951, 3.2.2): the symbols with a non-zero length, in (length, symbol) order, take increasing
 * code values.  A code's bits go most significant first into successive bit positions; position p is bit p % 64 of word
 * p / 64; the tail bits of the last word are 0.  A stream with one distinct symbol gives it length 1 and code 0; a stream
 * with nsym == 0 is mode 0 with no body.  The writer chooses mode 1 iff the mode-1 body, padding included, is strictly
 * smaller than the mode-0 body and nbits < 2^32: a coded file exceeds its "MCZW" twin by at most 16 bytes per stream.
 * The lengths are in the file (a length-limited Huffman code of the stream's histogram, compress.huffman_lengths): no
 * reader recomputes them.  A reader refuses lengths whose Kraft sum is not 1 (1/2 for a single symbol). */
#define MCAMD_HZ_MAXLEN 12
#define MCAMD_HZ_CHUNK 1024 /* symbols per chunk: one chunk_bit0 entry each */
#define MCAMD_HZ_GROUP 64   /* chunks per workgroup of the histogram and decode passes */

/* One stream of a pass.  All streams of a file go through ONE table: a HOST array for the checks and the grid sizes and
 * its DEVICE copy for the kernels.  Running sums over the table, in order (checked):
 *   block0 += ceil(ceil(nsym / MCAMD_HZ_CHUNK) / MCAMD_HZ_GROUP)
 *   chunk0 += ceil(nsym / MCAMD_HZ_CHUNK)        encode only
 * sym0, word0 and (decode) chunk0 are any offsets whose range lies inside the arrays given (checked before any launch). */
typedef struct mcamd_hz_seg {
    int64_t sym0;      /* byte offset of the stream's symbols in `syms` (histogram, encode: read) or `out` (decode: written),
                          a multiple of 8 */
    int64_t nsym;      /* symbols, >= 0.  histogram with `dyn`: the most the stream can have */
    int64_t nbits;     /* encode, decode: code bits of the stream, < 2^32 and <= MCAMD_HZ_MAXLEN nsym.  histogram: unused */
    int64_t word0;     /* encode, decode: first uint64 of the stream's code bits in `bits` */
    int64_t chunk0;    /* encode, decode: first entry of the stream in `chunk_bit0` */
    int64_t popc_bits; /* decode: > 0: the symbols are bit words (nsym a multiple of 8) of which the first popc_bits bits
                          stand for weights: stats gets their population count.  0: not counted.  Otherwise unused */
    int32_t block0;    /* first workgroup of the stream */
    int32_t A;         /* alphabet, 1..256: a symbol >= A has no code */
} mcamd_hz_seg;

/* workspace of histogram and encode for a table of `nseg` streams and `nblocks` workgroups (the final block0 sum) */
size_t mcamd_hz_workspace_bytes(int64_t nblocks, int32_t nseg);

/* hist[s][v] (uint64 [nseg][256]) = how many symbols of stream s are v.  Each workgroup counts its MCAMD_HZ_GROUP chunks in
 * LDS counters of its own; a second launch adds a stream's workgroups in workgroup order: integer counts in a fixed order,
 * a function of the input only.  `dyn` (device int64 [nseg][2], or NULL) gives sym0 and nsym of every stream from the
 * device, for symbols whose place a device pass before decided (mcamd_wz_pack's values): a pair that is negative, not a
 * multiple of 8, longer than the table's nsym or outside syms_bytes counts as an empty stream.  Not recordable. */
int mcamd_hz_histogram(const mcamd_hz_seg* segs, const mcamd_hz_seg* segs_dev, int32_t nseg, const uint8_t* syms,
                       int64_t syms_bytes, const int64_t* dyn, uint64_t* hist, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Encode: from the symbols and length (device uint8 [nseg][256], 0 = absent; a length above MCAMD_HZ_MAXLEN and a symbol
 * >= A count as absent and take no bits) the chunk_bit0 of every stream (chunk_bit0[chunk0 ...], chunk0 the running sum)
 * and its code bits (bits[word0 ...], ZERO `bits` first).  nbits is the caller's sum of hist[v] length[v]; no word behind
 * ceil(nbits / 64) is written.  Launches: per-chunk bit sums -> an exclusive scan per stream, which is the file's index
 * table -> the bits: a workgroup ORs its chunk's codes into LDS words and stores them, the first and last 32-bit word of a
 * chunk by an integer atomic OR.  Nothing floating-point, nothing order-dependent.  Not recordable. */
int mcamd_hz_encode(const mcamd_hz_seg* segs, const mcamd_hz_seg* segs_dev, int32_t nseg, const uint8_t* syms,
                    int64_t syms_bytes, const uint8_t* length, uint32_t* chunk_bit0, int64_t chunk_cap, uint64_t* bits,
                    int64_t bits_cap, void* workspace, size_t workspace_bytes, void* stream);

/* Decode: the symbols of stream s to out[sym0 ...], one lane per chunk through a 2^MCAMD_HZ_MAXLEN entry table of the stream
 * in LDS.  chunk_bit0 and bits are read where the caller has them (chunk0 in uint32, word0 in uint64 units: an uploaded
 * file serves as both).  A lane takes no bit at or past the end of its chunk (the next chunk's chunk_bit0; nbits for the
 * last chunk), loads no word behind ceil(nbits / 64) and stores nothing outside its chunk's min(1024, rest) symbols.
 * stats (device uint64 [nseg][2], cleared by the call): stats[s][0] bit 0 = a chunk of the stream did not end exactly at its
 * end or met an unassigned code (its remaining symbols are not written), bit 1 = a decoded bit word has a bit set at or
 * past popc_bits; stats[s][1] = the population count of the first popc_bits decoded bits.  Not recordable. */
int mcamd_hz_decode(const mcamd_hz_seg* segs, const mcamd_hz_seg* segs_dev, int32_t nseg, const uint8_t* length,
                    const uint32_t* chunk_bit0, int64_t chunk_cap, const uint64_t* bits, int64_t bits_cap, uint8_t* out,
                    int64_t out_bytes, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------------- *
 * Weight sharing (trained quantisation by k-means; an addition beyond the reference).
 * ------------------------------------------------------------------------- */
/* Per layer, over its KEPT weights (mask value != 0; every weight when the layer has no mask), K = 2^bits, bits 1..8.
 * The arithmetic, operation by operation (float64 unless said otherwise, no contraction):
 *   range    lo, hi = minimum and maximum of the kept fp32 weights.  A layer with no kept weight gets a codebook of K
 *            zeros; its codes are never read.
 *   init     c[k] = fp32(lo + ((hi - lo) * k) / (K - 1)), k = 0..K-1, in exactly that order (the linear initialisation).
 *   assign   code = the number of j in 0..K-2 with mid[j] < w, mid[j] = (double(c[j]) + double(c[j+1])) / 2, w widened to
 *            double: ties go to the lower index, equal centroids are harmless.  The codebook is non-decreasing (init
 *            makes it so and update keeps it so), so the count is found by bisection: np.searchsorted(mid, w, "left").
 *            Every operation is exact, so the codes are bit-exact given the centroids.
 *   update   per cluster, sum = the float64 sum of its members, count = their number; c[k] = fp32(sum / count); an empty
 *            cluster keeps its centroid.  No floating-point atomics: the layer is cut into slabs of MCAMD_WS_SLAB
 *            consecutive weights, one workgroup sums one slab in a fixed order, and the slab sums are added in slab
 *            order.  Order inside a slab, for cluster k: the slab is cut into S = 256 / K sub-slabs of MCAMD_WS_SLAB / S
 *            consecutive weights; each sub-slab's members are added in index order starting from 0.0, then the S sub-slab
 *            sums are added in sub-slab order starting from 0.0.  The result is bit-reproducible from run to run.
 *   kmeans   init, `iters` rounds of assign then update, and one last assign against the codebook returned.
 *   project  with the codes fixed: update, then w = c[code] on every kept weight.  Weights that are not kept are not
 *            written; an empty cluster changes nothing.  `count` copies of one fp32 value sum exactly in float64 for
 *            count <= 2^29 whatever the order, so on a layer that is already tied the projection is the identity, bit
 *            for bit.
 *   expand   w = c[code] on kept weights and +0 elsewhere.
 * tests/wshare_ref.py restates this in numpy. */
#define MCAMD_WS_SLAB 4096 /* weights per workgroup */

/* One layer of a pass.  All layers go through ONE table: a HOST array for the checks and the grid size and its DEVICE
 * copy for the kernels.  Running sums over the table, in order (checked):
 *   slab0  += ceil(n / MCAMD_WS_SLAB)
 *   cb0    += K                             the layer's K entries in `codebook`, `sums` and `counts`
 *   part0  += ceil(n / MCAMD_WS_SLAB) * K   the layer's slab sums in the workspace
 * w and mask are 16-byte aligned, codes 4-byte aligned (checked). */
typedef struct mcamd_ws_seg {
    void* w;        /* fp32 [n]: read by init / iterate / assign, read and written by project, written by expand */
    void* mask;     /* fp32 0/1 mask, or NULL = every weight is kept */
    void* codes;    /* uint8 [n]: written by iterate / assign, read by project / expand; codes of weights that are not
                       kept are written as 0 and never read.  init alone takes NULL */
    int64_t n;      /* weights, > 0 */
    int64_t part0;
    int32_t K;      /* 2, 4, 8, ..., 256 */
    int32_t cb0;
    int32_t slab0;
    int32_t reserved;
} mcamd_ws_seg;

/* workspace of every pass below for a table of `nseg` layers, `nslabs` slabs and `parts` slab sums (the final sums) */
size_t mcamd_ws_workspace_bytes(int64_t nslabs, int64_t parts, int32_t nseg);

/* range + init: codebook[cb0 + k] of every layer.  cb_cap = entries of `codebook` (and of `sums` / `counts` below). */
int mcamd_ws_init(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, float* codebook, int64_t cb_cap,
                  void* workspace, size_t workspace_bytes, void* stream);
/* One round: assign against `codebook` (codes written), then update `codebook` in place.  sums[cb0 + k] (float64) and
 * counts[cb0 + k] (int64) receive the cluster sums and sizes of the round.  Called `iters` times with nothing read back. */
int mcamd_ws_iterate(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, float* codebook, int64_t cb_cap,
                     double* sums, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
/* assign alone: the codes against `codebook`. */
int mcamd_ws_assign(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, const float* codebook, int64_t cb_cap,
                    void* stream);
/* project: `codebook` is updated in place to the cluster means and written back to the kept weights.  One call for the
 * whole model, no read-back: the training step calls it behind every optimizer step. */
int mcamd_ws_project(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, float* codebook, int64_t cb_cap,
                     double* sums, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
/* expand: w = codebook[code] on kept weights, +0 elsewhere.  A code >= K reads entry K - 1 (never outside the layer's). */
int mcamd_ws_expand(const mcamd_ws_seg* segs, const mcamd_ws_seg* segs_dev, int32_t nseg, const float* codebook, int64_t cb_cap,
                    void* stream);

/* ------------------------------------------------------------------------- *
 * First-order Taylor importance (taylor_prune; an addition beyond the reference; Molchanov et al. 2019,
 * arXiv:1906.10771): the importance of a group S of parameters is (sum over S of g w)^2, summed over training steps.  One
 * call between backward() and optimizer.step() adds one step's term to every accumulator of every layer: one launch over
 * a segment table, nothing read back, no atomics, every result a function of the operands alone.
 * ------------------------------------------------------------------------- */
/* A CONV segment is one conv layer: w and g (its gradient) fp32 OIHW [cout][cin][khw], optionally its bias and the bias's
 * gradient fp32 [cout] (both or neither).  With p_i = g_i * w_i rounded to fp32 (one multiply, no contraction), its three
 * optional outputs -- a NULL one is neither computed nor written -- are
 *   acc_w  fp32 [cout cin khw]   acc_w[i] = acc_w[i] + p_i * p_i, both operations rounded to fp32
 *   acc_b  float64 [blocks]      cin % 32 == 0 only; the blocks and the block index of mcamd_block_scores (64 filters x kb
 *                                channels x one tap, kb = 64 when cin % 64 == 0 else 32, ragged last filter block, index
 *                                (fb * (cin / kb) + cb) * khw + tap).  S_b = the float64 sum of (double)p_i over the block in
 *                                that function's order: elements numbered e = r * kb + c, lane l adds e = l, l + 64, ... in
 *                                ascending order starting from 0.0, the 64 lane sums are combined by s[l] += s[l ^ d],
 *                                d = 32, 16, 8, 4, 2, 1.  Then acc_b[b] = acc_b[b] + S_b * S_b: one rounded multiply, one
 *                                rounded add.
 *   acc_f  float64 [cout]        for a conv WITHOUT BatchNorm.  S_f = the float64 sum of (double)p_i over filter f with the
 *                                elements in memory order, e = c * khw + tap, and the same lane and butterfly order; then
 *                                S_f = S_f + (double)(gbias_f * bias_f) (the product rounded to fp32) when there is a bias;
 *                                acc_f[f] = acc_f[f] + S_f * S_f.
 * A GATE segment is one BatchNorm: w = gamma, g = dgamma, bias = beta, gbias = dbeta, fp32 [cout], cin = khw = 1, acc_f only:
 *   t = (double)gamma * (double)dgamma + (double)beta * (double)dbeta (the products are exact, the sum is rounded once);
 *   acc_f[c] = acc_f[c] + t * t.
 * A conv followed by BatchNorm on batch statistics takes its filter scores from the gate: the loss does not change when
 * such a filter is rescaled, so its own sum of g w is zero up to rounding (Euler's theorem).
 * fp32 arrays are 4-byte aligned (a gradient may be a view into a flat buffer), float64 arrays 8-byte aligned (checked).
 * tests/taylor_ref.py restates this in numpy. */
#define MCAMD_TAYLOR_CONV 0
#define MCAMD_TAYLOR_GATE 1
typedef struct mcamd_taylor_seg {
    void* w;        /* conv: weights; gate: gamma */
    void* g;        /* conv: weight gradient; gate: dgamma */
    void* bias;     /* conv: bias or NULL; gate: beta */
    void* gbias;    /* conv: bias gradient or NULL; gate: dbeta */
    void* acc_w;    /* read and written; NULL = not wanted */
    void* acc_b;
    void* acc_f;
    int64_t wg0;    /* running sum over the table of mcamd_taylor_seg_workgroups (checked) */
    int32_t kind;   /* MCAMD_TAYLOR_CONV / MCAMD_TAYLOR_GATE */
    int32_t cout;   /* gate: channels */
    int32_t cin;    /* gate: 1 */
    int32_t khw;    /* gate: 1 */
} mcamd_taylor_seg;

/* workgroups the launch spends on one segment (wg0 is ignored); 0 for a segment mcamd_taylor_accum refuses by its shape */
int64_t mcamd_taylor_seg_workgroups(const mcamd_taylor_seg* seg);

/* One step of every segment.  `segs` is a HOST array for the checks and the grid size, `segs_dev` its DEVICE copy for the
 * kernel.  skip: device fp32 scalar or NULL; when *skip != 0 nothing is accumulated and *steps is left alone (train.StepGuard's
 * `found`: an overflowed or non-finite step adds nothing).  Otherwise *steps (device int32) = *steps + 1.  Launch-type:
 * recorded into a launch plan while one is being recorded.  Refused without a launch (MCAMD_EINVAL): NULL or misaligned
 * pointers, acc_b with cin % 32 != 0, a gate with acc_w / acc_b, a conv segment without any output, a wg0 that is not the
 * running sum. */
int mcamd_taylor_accum(const mcamd_taylor_seg* segs, const mcamd_taylor_seg* segs_dev, int32_t nseg, const float* skip,
                       int32_t* steps, void* stream);

/* ------------------------------------------------------------------------- *
 * Proximal group lasso (sparsify.GroupLasso; an addition beyond the reference; Wen et al. 2016,
 * arXiv:1608.03665, for weight groups; Liu et al. 2017, arXiv:1708.06519, for BatchNorm gates): the proximal step of a
 * group-lasso penalty, taken behind optimizer.step().  A group the loss does not need shrinks to exactly zero over the
 * steps.  One launch over a segment table for the whole model, nothing read back, no atomics, every written element has
 * one owner, every result a function of the operands alone.
 * ------------------------------------------------------------------------- */
/* A BLOCK segment is one conv weight, fp32 OIHW [cout][cin][khw], cin % 32 == 0.  Its groups are the blocks of
 * mcamd_block_scores with that function's block index: filters [64 fb, min(64 fb + 64, cout)) x kb channels x one tap, kb = 64
 * when cin % 64 == 0 else 32, index (fb * (cin / kb) + cb) * khw + tap.  For a block of n_g elements:
 *   n2    the float64 sum of (double)w_i * (double)w_i (each product is exact) in that function's order: elements numbered
 *         e = r * kb + c, lane l adds e = l, l + 64, ... in ascending order starting from 0.0, the 64 lane sums are
 *         combined by s[l] += s[l ^ d], d = 32, 16, 8, 4, 2, 1
 *   thr2  = tau2 * (double)n_g, one rounded multiply
 *   n2 <= thr2:  every element of the block becomes +0.0f
 *   otherwise:   s = 1.0 - sqrt(thr2 / n2) in float64 (one divide, one square root, one subtract), and
 *                w_i = (float)((double)w_i * s)
 * which is the proximal operator of lam * sqrt(n_g) * ||w_g||_2 at step lr when tau2 = (lr * lam)^2.  Non-finite values
 * are not hidden: a block that holds an Inf keeps its values (n2 = Inf, s = 1), a block that holds a NaN becomes NaN
 * (n2 <= thr2 is false, s is NaN).  nz (int32 [blocks], or NULL = not written): 0 when n2 <= thr2, else 1.
 * A GATE segment is one BatchNorm weight, fp32 [cout], cin = khw = 1:
 *   a = fabsf(gamma) - tau_gate, one fp32 subtract; gamma = copysignf(a, gamma) when a > 0, +0.0f when a <= 0, and
 *   gamma is left alone when a is NaN.  nz (int32 [cout] or NULL): 0 when a <= 0, else 1.
 * No |w| and no |gamma| grows.  All arrays are 4-byte aligned (checked).  tests/gprox_ref.py restates this in numpy. */
#define MCAMD_GPROX_BLOCK 0
#define MCAMD_GPROX_GATE 1
typedef struct mcamd_gprox_seg {
    void* w;        /* block: weights; gate: gamma.  Read and written */
    void* nz;       /* int32, one entry per group; NULL = not wanted */
    int64_t wg0;    /* running sum over the table of mcamd_gprox_seg_workgroups (checked) */
    int32_t kind;   /* MCAMD_GPROX_BLOCK / MCAMD_GPROX_GATE */
    int32_t cout;   /* gate: channels */
    int32_t cin;    /* gate: 1 */
    int32_t khw;    /* gate: 1 */
} mcamd_gprox_seg;

/* workgroups the launch spends on one segment (wg0 is ignored); 0 for a segment mcamd_group_prox refuses by its shape */
int64_t mcamd_gprox_seg_workgroups(const mcamd_gprox_seg* seg);

/* One proximal step of every segment.  `segs` is a HOST array for the checks and the grid size, `segs_dev` its DEVICE copy
 * for the kernel.  tau2 applies to the BLOCK segments, tau_gate to the GATE segments; the caller passes (lr * lam)^2 and
 * (float)(lr * lam).  skip: device fp32 scalar or NULL; when *skip != 0 nothing is written at all, neither weights nor
 * flags (train.StepGuard's `found`: a skipped optimizer step leaves the weights as they were).  Launch-type: recorded into a
 * launch plan while one is being recorded.  Refused without a launch (MCAMD_EINVAL): NULL or misaligned pointers, a BLOCK
 * segment with cin % 32 != 0, a GATE segment that is not [C][1][1], a wg0 that is not the running sum, a negative or
 * non-finite tau2 or tau_gate. */
int mcamd_group_prox(const mcamd_gprox_seg* segs, const mcamd_gprox_seg* segs_dev, int32_t nseg, double tau2, float tau_gate,
                     const float* skip, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MCAMD_H */
