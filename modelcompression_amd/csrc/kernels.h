// Internal launch descriptors shared between the kernel translation units and api.hip.
#pragma once
#include "common.h"

// BatchNorm-backward sums of the PLAIN block whose output gradient G a dgrad launch stores (mcamd_dgrad_sums, mcamd.h;
// conv_epi.h store_raw_tile_sums): pass 0 of bn_plain_bwd_kernel<., BN_SRC_ACT> taken on the fp16 tile on its way out.
struct DgradSums {
    float* slab;             // [num_pslots][2][ld]: sum g_z, sum g_z xhat per producer channel; NULL = none
    const half_t* act;       // the producer's stored activation (padded NHWC / shared-halo form per act_pw)
    const float* scale;
    const float* shift;
    const float* mean;
    const float* invstd;
    const float* y;          // the producer's saved fp32 raw output [M][y_ld] (ill-conditioned channels only) or NULL
    int act_ld, act_choff, act_pw;   // producer channel c of a pixel: act[pad_off(..) + act_choff + c]
    int y_ld, y_choff;
    int ch_lo, C;            // the producer's channels are the G columns [ch_lo, ch_lo + C)
    int ld;
    float slope;
};
// Kernel-instance selector beside the MCAMD_EPI_* modes (never in IgemmArgs.mode): MCAMD_EPI_RAW_F16 with a.bsum taken
#define MCAMD_EPI_RAW_F16_SUMS 4

struct IgemmArgs {
    const half_t* x;
    const half_t* w;
    void* y;
    const float* bias;
    float* stats;
    const float* scale;
    const float* shift;
    long long x_img_stride;  // elements between images of x
    int x_row_stride;        // elements between padded rows of x
    int x_ld;                // elements per pixel of x
    int x_off;               // channel offset added to every row base
    int H, W, HW, M, N;
    int ktot;                // ntaps * cin_tap
    int cin_tap;
    int ntaps;
    int kb;                  // channel-block size of the packed K order [cb][tap][kb]: 64 when cin_tap % 64 == 0, else 32
    int tap_off[9];          // element offset of tap t from the row base
    int mode;
    int y_ld, y_choff;
    int stats_ld;
    float slope;
    int num_mtiles;
    int num_pslots;  // persistent workgroups along M (= rows of the statistics slab)
    int num_ntiles;
    int xcd_order;
    int* overflow;   // optional: set to 1 when an fp16 output was clamped to +-65504
    // inference epilogue fused with MaxPool(2,2) / Reorg(2) (MCAMD_EPI_PAD_F16 only, conv_epi.h): dst_mode != 0 enumerates
    // the M tile in pooled order and `y` is at the pooled resolution; y2 = optional full-resolution copy (POOL)
    int dst_mode;
    void* y2;
    int y2_ld, y2_choff;
    int concurrent;  // mcamd_conv_epilogue.concurrent (dgrad): tiles chosen for CU-time, see pick_tile
    int wrap;        // mcamd_conv_geom.x_wrap (INT_MAX = none): channel blocks >= wrap are read `wrap` channels lower
    int f8_from;     // mcamd_conv_geom.x_f8: first K chunk (of 32 fp16 = 64 e4m3 values) of the fp8 correction part; INT_MAX = none
    int f8_sb;       // e8m0 scale of the B operand of the fp8 MFMAs in all four bytes: 2^-(F8_SXL + x_f8_wexp) (A: 1.0)
    DgradSums bsum;  // dgrad, mode MCAMD_EPI_RAW_F16: bsum.slab != NULL selects the MCAMD_EPI_RAW_F16_SUMS instances
};


struct StemArgs {        // conv_stem.hip: forward of the 3-channel first layer
    const half_t* x;     // padded NHWC4 image
    const half_t* w;     // packed stem weights [Npad][96]
    half_t* y;           // raw output [M][y_ld]
    float* stats;        // [grid][2][stats_ld] or NULL
    int y_ld, y_choff, stats_ld;
    int H, W, HW, M;
};

struct WgradArgs {
    const half_t* x;
    const half_t* dy;
    float* slab;
    long long x_img_stride, dy_img_stride;
    int x_row_stride, dy_row_stride, x_ld, dy_ld;
    int x_off;        // channel offset of x
    int dy_off;       // channel offset of dy + offset of padded pixel (1,1)
    int dy_zero_off;  // channel offset of dy at padded pixel (0,0): a zero row
    int H, W, HW, M;
    int rows_pad;     // slab rows
    int ktot, cin_tap, ntaps;
    int tap_off[9];
    int n_ctiles;     // cin tiles per tap
    int n_otiles, n_tapgroups, nsplit;
    int pix_per_split;
    const int* tile_list;   // list launch (mcamd_conv_wgrad_bsparse): the tile indices ot * n_ctiles + ct to run, n_list of them
    int n_list;
};

struct WgradPlan {
    int tmo, tnc, taps, kp, rows_pad, n_otiles, n_ctiles, n_tapgroups, nsplit, pix_per_split;
    int nine;   // 1: padded-pixel 9-tap kernel (wgrad9_kernel), 2: its wide form (wgrad9w_kernel)
    int stemw;  // 1: raw-window first-layer kernel (wgrad_stem_kernel), 2: raw-window 32-channel kernel (wgrad_win_kernel)
    int ns;     // LDS ring stages of the kernel instance (the NS template argument where the kernel has one)
    size_t bytes;
};

// Which kernel sums the split-K slabs into dW (mcamd_wgrad_finish_launch) and how many lanes share one sum.
struct WgradFinish {
    int kernel;   // MCAMD_WFIN_ROW: wgrad_finish_row_kernel, _VEC: wgrad_finish_vec_kernel, _GENERIC: wgrad_finish_kernel
    int sg;       // the SG template argument (1 / 8 / 32); 0 for the row kernel, which has none
};

// Which kernel a forward / dgrad launch takes, its workgroup tile and the rows of the statistics slab it writes: decided
// once per launch or query by conv_route() (api.hip).  `kernel` = the kinds of mcamd_conv_tile_info (mcamd.h).
enum { ROUTE_IGEMM = 0, ROUTE_STEM = 1, ROUTE_PP = 2, ROUTE_SMALL3X3 = 4, ROUTE_WIN3X3 = 5, ROUTE_WRES = 6, ROUTE_SMALL3X3_SPLIT = 7 };
struct ConvRoute {
    int kernel;
    int bm, bn, bk;
    int rows;   // persistent workgroups along M
};

// conv_igemm.hip: pick_tile + the persistent-workgroup count for an implicit GEMM of M pixels x n channels (kernel
// ROUTE_IGEMM, ROUTE_PP or ROUTE_SMALL3X3); mcamd_igemm_launch takes the first two as given
ConvRoute mcamd_igemm_route(long long M, int n, int cin_tap, int ktot, bool raw_epilogue, bool concurrent);
int mcamd_igemm_pp_launch(const IgemmArgs& a, int bm, int bn, int rows, int ntiles, hipStream_t st);
int mcamd_igemm_launch(IgemmArgs& a, const ConvRoute& r, hipStream_t st);
bool mcamd_igemm_sums_ok(const ConvRoute& r);   // the route's kernel has a MCAMD_EPI_RAW_F16_SUMS instance (IgemmArgs.bsum)
// conv_splitk.hip: split-K forward (partial + finish launch).  mcamd_splitk_plan is the tile and the slice policy
// (forced > 0: that slice count instead of the policy's); slab_elems = floats per slice of the workspace
struct SplitkPlan {
    int bm, bn, bk, chunks, mtiles, ntiles, tiles, slices;
    int stages;   // LDS ring depth of the partial kernel instance
    int fr, fc;   // finish tile: pixels x channels
    long long slab_elems;
};
SplitkPlan mcamd_splitk_plan(long long M, int n, int cin_tap, int ktot, int forced);
int mcamd_splitk_launch(const IgemmArgs& a, const SplitkPlan& p, float* ws, hipStream_t st);
// conv_bsparse.hip: the K chunks of each 64-filter N tile from a list (count[ntiles], list[ntiles][ktot / kb]), mode 2
// epilogue (inference) or mode 0 (a.mode == MCAMD_EPI_RAW_F16: the training form, forward and dgrad; a.stats: one slab row
// per pixel tile); and the lists of a packed forward or dgrad weight matrix
#define MCAMD_BSPARSE_BM_DEFAULT 128
// mcamd_bsparse_choice names the bsparse_kernel instance (bm pixels x bn filters, K chunks of bk, LDS ring stages) and its
// grid (whole rounds of 8 pixel tiles) for M pixels x N filters with channel blocks of kb; the launch dispatches on it
struct BsparseChoice {
    int bm, bn, bk, stages, mtiles, ntiles, grid;
};
BsparseChoice mcamd_bsparse_choice(long long M, int N, int kb);
int mcamd_bsparse_launch(IgemmArgs& a, const int* count, const int* list, hipStream_t st);
int mcamd_bsparse_lists_launch(const void* wp, int cout, int cin_tap, int ntaps, int* count, int* list, hipStream_t st);
// conv_sparse.hip: 2:4 weights, mode 2 epilogue.  mcamd_sparse24_choice names the sparse24_kernel instance (bmw filters x
// bnp pixels, K chunks of bk, LDS ring stages) and its grid for M pixels x N filters with channel blocks of kb; the launch
// dispatches on it
struct Sparse24Choice {
    int bmw, bnp, bk, stages, mtiles, ntiles, grid;
};
Sparse24Choice mcamd_sparse24_choice(long long M, int N, int kb);
int mcamd_sparse24_launch(IgemmArgs& a, const void* idx, hipStream_t st);
int mcamd_pack_sparse24_launch(const float* w, const float* mask, void* vals, void* idx, int cout, int cin, int ntaps,
                               int cin_tap, int kb, hipStream_t st);
// conv_q8.hip / conv_q8_sparse.hip: mcamd_q8_choice names the conv_q8_kernel / conv_q8_border_kernel / conv_q8_sparse_kernel
// instance (bmw filters x bnp pixels, the MFMA form MCAMD_Q8_MFMA selects, LDS ring stages) and its grid for M pixels x N
// filters in one of the four forms; both launches dispatch on it
#define MCAMD_Q8_FORM_INFER 0    // conv_q8_kernel, inference epilogue
#define MCAMD_Q8_FORM_RAW 1      // conv_q8_kernel, raw fp32 epilogue + statistics (fp8-qat; conv_q8_w4_raw_kernel under fp8-w4-qat)
#define MCAMD_Q8_FORM_BORDER 2   // conv_q8_border_kernel (slim models with a border table)
#define MCAMD_Q8_FORM_SPARSE 3   // conv_q8_sparse_kernel (2:4)
struct Q8Choice {
    int bmw, bnp, f8mfma, stages, mtiles, ntiles, grid;
};
Q8Choice mcamd_q8_choice(long long M, int N, int form);
// conv_q8.hip: e4m3 operands (byte strides in `a`), mode 2 epilogue with a format per destination; packer; cast pass
// (`border`: fp32 [16][border_ld] table the inference epilogue adds by pixel class, mcamd_conv_fwd_q8_slim; NULL = none)
int mcamd_conv_q8_launch(IgemmArgs& a, const void* wexp, int y_f8, int y2_f8, hipStream_t st, const float* border = nullptr,
                         int border_ld = 0);
int mcamd_pack_q8_launch(const float* w, const float* mask, void* wq, void* wexp, int cout, int cin, int ntaps, hipStream_t st);
// ... rows of round_up(cin, 64) channels per tap, zero bytes behind the real ones (cin % 8 == 0)
int mcamd_pack_q8_slim_launch(const float* w, const float* mask, void* wq, void* wexp, int cout, int cin, int ntaps, hipStream_t st);
// (a.mode MCAMD_EPI_RAW_F32: the training form, fp32 y + one statistics row per pixel tile of MCAMD_Q8_TILE_M pixels)
#define MCAMD_Q8_TILE_M 128
int mcamd_cast_q8_launch(const void* src, long long pixels, int src_ld, int src_choff, int C, void* dst, int dst_ld,
                         int dst_choff, int back, hipStream_t st);
int mcamd_fakequant_q8_launch(const float* w, const float* mask, const void* wexp, float* out, int cout, int cin, int ntaps,
                              hipStream_t st);
// conv_q8_splitk.hip: split-K pair on conv_q8.hip's operands (partial + finish launch, mode 2 epilogue).  `p`: mcamd_splitk_plan
// for 64-wide chunks (cin % 64 == 0); ws: p.slices * p.slab_elems floats; the MFMA form is mcamd_q8_choice's
int mcamd_q8_splitk_launch(const IgemmArgs& a, const SplitkPlan& p, const void* wexp, int y_f8, int y2_f8, float* ws, hipStream_t st);
// conv_q8_bsparse.hip: conv_q8.hip's K loop (conv_q8_loop.h) on a 64 x 128 tile over the K chunks each 64-filter tile lists (count[ntiles],
// list[ntiles][ktot / 64]); its instance and grid; the lists of mcamd_pack_q8's bytes
Q8Choice mcamd_q8_bsparse_choice(long long M, int N);
int mcamd_conv_q8_bsparse_launch(IgemmArgs& a, const void* wexp, const int* count, const int* list, int y_f8, int y2_f8, hipStream_t st);
int mcamd_q8_bsparse_lists_launch(const void* wq, int cout, int cin, int ntaps, int* count, int* list, hipStream_t st);
// conv_q8_sparse.hip: conv_q8.hip's K loop and epilogue (conv_q8_loop.h) on 2:4-compressed e4m3 weights (sparse MFMA); packer
int mcamd_conv_q8_sparse_launch(IgemmArgs& a, const void* idx, const void* wexp, int y_f8, int y2_f8, hipStream_t st);
int mcamd_pack_q8_sparse24_launch(const float* w, const float* mask, void* wq, void* idx, void* wexp, int cout, int cin,
                                  int ntaps, hipStream_t st);
// conv_q8_w4.hip: conv_q8.hip's K loop and epilogue (conv_q8_loop.h) on e2m1 codes + group shifts expanded to e4m3 bytes in
// registers (a.w = the codes);
// its choice of instance (the fp8 block's), packer, expander to mcamd_pack_q8's bytes
Q8Choice mcamd_q8_w4_choice(long long M, int N);
int mcamd_conv_q8_w4_launch(IgemmArgs& a, const void* gshift, const void* wexp, int y_f8, int y2_f8, hipStream_t st);
int mcamd_pack_q8_w4_launch(const float* w, const float* mask, void* codes, void* gshift, void* wexp, int cout, int cin, int ntaps,
                            hipStream_t st);
int mcamd_unpack_q8_w4_launch(const void* codes, const void* gshift, void* wq, int cout, int cin, int ntaps, hipStream_t st);
// ... its training form (a.mode MCAMD_EPI_RAW_F32: the raw fp8 block's tile, fp32 y + one statistics row per pixel tile), and the
// fp32 OIHW values the codes stand for
int mcamd_conv_q8_w4_raw_launch(IgemmArgs& a, const void* gshift, const void* wexp, hipStream_t st);
int mcamd_fakequant_q8_w4_launch(const void* codes, const void* gshift, const void* wexp, float* out, int cout, int cin, int ntaps,
                                 hipStream_t st);

WgradPlan mcamd_wgrad_plan(long long M, int cout, int cin_tap, int ntaps);
int mcamd_wgrad_launch(WgradArgs& a, const WgradPlan& p, hipStream_t st);
bool mcamd_wgrad_stem_ok(int stem, int cout, int W, long long M);   // conv_wgrad_stem.hip
WgradPlan mcamd_wgrad_stem_plan(long long M);
int mcamd_wgrad_stem_launch(WgradArgs& a, const WgradPlan& p, hipStream_t st);
bool mcamd_wgrad_win_ok(int ksize, int stem, int cout, int cin_tap, int W, long long M);
WgradPlan mcamd_wgrad_win_plan(long long M, int cout);
int mcamd_wgrad_win_launch(WgradArgs& a, const WgradPlan& p, hipStream_t st);
bool mcamd_wgrad_use9(int ksize, int stem, int cout, int cin_tap, int W);
WgradPlan mcamd_wgrad_plan9(long long P, int cout, int cin_tap, int W, int pitch, int B);
int mcamd_wgrad9_launch(const WgradArgs& w, const WgradPlan& p, int pitch, long long P, hipStream_t st);
WgradFinish mcamd_wgrad_finish_pick(int nsplit, int stem, int Cin, int ksize, bool has_cmap);
int mcamd_wgrad_instances(int (*out)[4], int cap);   // the (TMo, TNc, TAPS, KP) of every wgrad_kernel instance; returns their number
int mcamd_wgrad_finish_launch(const float* slab, const WgradPlan& p, int ktot, int cin_tap, int stem, int Cout, int Cin,
                              int ksize, const float* mask, float inv_scale, float* dw, const int* rmap, const int* cmap,
                              hipStream_t st, bool select = false);
// the list launch of the two 64 x 64 kernels (mcamd_conv_wgrad_bsparse): `nsplit` 0 asks the cost rule for `kept_tiles` tiles
bool mcamd_wgrad_bsparse_ok(int ksize, int stem, int cout, int cin, int W);
WgradPlan mcamd_wgrad_bsparse_plan(int ksize, long long M, long long P, int cout, int cin, int pitch, int kept_tiles, int nsplit);
int mcamd_wgrad_bsparse_lists_launch(const float* mask, int cout, int cin, int kk, int* tiles, int* words, int* counts, hipStream_t st);
int mcamd_wgrad_bsparse_launch(WgradArgs& a, const WgradPlan& p, int pitch, long long P, const int* tiles, const int* words,
                               int ntiles, hipStream_t st);
int mcamd_colsum_launch(const half_t* dy, long long rows, int ld, int choff, int C, float inv_scale, float* out,
                        hipStream_t st, void* scratch, size_t scratch_bytes);   // scratch: reusable once the finish pass is enqueued

// conv_bwd1x1.hip: dgrad + producer sums + wgrad of a dense 1x1 block in one persistent launch (mcamd_conv_bwd1x1).  The grid
// is fixed: it is the number of sums rows and of dW splits, and one workgroup fits a CU.
#define MCAMD_BWD1X1_GRID 256
struct Bwd1x1Launch {
    const half_t* dy;
    const half_t* x;
    const half_t* w;     // dgrad packing [cin][cout]
    half_t* g;           // raw [M][g_ld]
    float* slab;         // [MCAMD_BWD1X1_GRID][cout][cin]
    int* overflow;
    int dy_ld, dy_choff, x_ld, x_choff, g_ld, g_choff;
    int H, W, M, pw, cout, cin;
    DgradSums bsum;      // slab NULL = none; the activation fields are not read (the activation is x)
};
const char* mcamd_bwd1x1_refusal(int ksize, int stem, int x_wrap, int x_f8, int cout, int cin);   // NULL: an instance exists
int mcamd_bwd1x1_launch(const Bwd1x1Launch& q, hipStream_t st);

// the per-kernel eligibility rules and slab rows conv_route() asks, each once; the launches take `rows` from the route
bool mcamd_win3x3_ok(int mode, bool stats, long long M, int n, int cin_tap, int ktot, int H, int W);   // conv_win.hip
int mcamd_win3x3_launch(const IgemmArgs& a, hipStream_t st);
bool mcamd_small3x3_ok(long long M, int n, int cin_tap, int ktot);   // conv_small.hip
int mcamd_small3x3_rows(long long M);
int mcamd_small3x3_launch(const IgemmArgs& a, int rows, hipStream_t st);
bool mcamd_small3x3_split_ok(long long M, int n, int cin_tap, int ktot, int wrap, int mode);   // split operands, fp32 output
int mcamd_small3x3_split_launch(const IgemmArgs& a, int rows, hipStream_t st);

// bn_conv1x1.hip: a PLAIN block's BatchNorm + LeakyReLU fused into the split-operand 1x1 forward behind it.  Not a route of
// conv_route(): its own entry point (mcamd_bn_act_conv1x1_fwd).  `a` as for the consumer's igemm launch + the producer's
// scale / shift / slope; py = the producer's fp32 raw output, P its channels
bool mcamd_bn_conv1x1_shape_ok(int P, int cout);
// the instance bn_conv1x1_kernel<bn, cb> and the launch dimensions of a pair (M pixels, `rows` persistent slots); false: none
struct BnConv1x1Choice { int bn, cb, threads, rows, num_mtiles, grid, lds_bytes; };
bool mcamd_bn_conv1x1_choice(int P, int cout, long long M, int rows, BnConv1x1Choice* c);
int mcamd_bn_conv1x1_launch(IgemmArgs& a, const float* py, int py_ld, int py_choff, int P, int rows, hipStream_t st);

bool mcamd_wres_ok(int ksize, int stem, int n, int cin_tap, int ktot, int B, int H, int W, int mode);   // conv_wres.hip
int mcamd_wres_rows(int n, int B, int H, int W);
int mcamd_wres_launch(IgemmArgs& a, int B, int rows, hipStream_t st);

bool mcamd_stem_direct_ok(int stem, int cout, int mode);
int mcamd_stem_rows(long long M);
int mcamd_stem_launch(const StemArgs& a, int cout, int rows, hipStream_t st);
