/*
 * stif.h -- C ABI of libstif_hip.so, the MI355X (gfx950) engine for the STIF
 * LunaTokis forward (reference: codes/models/modules/Sakuya_arch_test.py).
 *
 * Conventions (every entry point):
 *   - plain device pointers (fp32), sizes as ints; no framework types;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - outputs and workspaces are caller-allocated; nothing allocates per call;
 *   - stateless and reentrant; returns 0 on success or a STIF_E_* code, with a
 *     message retrievable through stif_last_error() (thread-local);
 *   - feature maps are NHWC ([item][y][x][channel]) unless a name says NCHW.
 *
 * The drop-in for the reference's native operator is stif_dcn_v2_forward; it
 * replaces `_ext.dcn_v2_forward` (DCNv2/src/vision.cpp:4, declared
 * DCNv2/src/dcn_v2.h:9-23, CUDA body DCNv2/src/cuda/dcn_v2_cuda.cu:42-172).
 * The remaining entry points are the fused stages the engine's LunaTokis host
 * (stif_amd.model) drives; INTEGRATION.md shows the reference-side bindings.
 */
#ifndef STIF_H
#define STIF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  STIF_OK = 0,
  STIF_E_INVALID = 1,   /* bad argument / unsupported shape */
  STIF_E_LAUNCH = 2,    /* kernel launch failed */
  STIF_E_WORKSPACE = 3, /* workspace too small */
  STIF_E_RANGE = 4      /* STIF_PACK_F16X3 packing: a weight exceeds the split-fp16 range (pack in fp32) */
};

/* activation / epilogue selector of stif_conv2d_nhwc and stif_dcn_nhwc */
enum {
  STIF_EPI_NONE = 0,
  STIF_EPI_LRELU = 1,   /* LeakyReLU(0.1)  (Sakuya_arch_test.py:69) */
  STIF_EPI_RELU = 2,    /* ReLU            (module_util.py:51) */
  STIF_EPI_RES = 3,     /* out = res + conv (ResidualBlock_noBN, module_util.py:48-52) */
  STIF_EPI_OFFMASK = 4, /* sigmoid on the mask channels of a DCN offset/mask conv (dcn_v2.py:134-138) */
  STIF_EPI_LSTM = 5     /* ConvLSTMCell gates (convlstm.py:47-56): out=h_next, out2=c_next, res=c_cur */
};

#define STIF_MAX_GROUPS 16

/* Item counts per weight set (stif_conv_args, stif_dcn_args, stif_dcn_sep_args).  A launch covers `ngroups` weight
 * sets (at most STIF_MAX_GROUPS); set g holds items [item_base[g], item_base[g + 1]) of the launch, so its own count
 * is item_base[g + 1] - item_base[g], and item i of set g uses in[g] + i * in_item (one item stride per operand and
 * launch, whatever the counts).  item_base is a prefix array: item_base[0] = 0, strictly increasing up to
 * item_base[ngroups]; entries past it are ignored.  A table of all zeros is the uniform form: every set holds
 * `nitems` items (nitems is not read otherwise).  STIF_E_INVALID before any launch: a table that does not start at
 * 0 or does not increase (an empty set), more than STIF_MAX_GROUPS sets, a total the launch grid cannot hold.  The
 * kernels find a workgroup's (set, item) by a scan of the prefix entries in scalar registers, once per tile. */

/* Direct/implicit-GEMM convolution on NHWC fp32 maps (replaces nn.Conv2d in the
 * hot path).  The input is the channel concatenation [in0 | in1] (so torch.cat
 * never materialises); in1 may be read through a fused bilinear x2 upsample
 * (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) times
 * in1_scale, Sakuya_arch_test.py:86-87).  A launch covers `ngroups` weight sets
 * x `nitems` items per set (item i of set g uses in0[g] + i*in0_item, ...), or
 * with `item_base` a count of its own per set (see STIF_MAX_GROUPS).
 * Weights are packed by stif_pack_conv_weight. */
typedef struct {
  const float* in0[STIF_MAX_GROUPS];
  const float* in1[STIF_MAX_GROUPS];
  const float* w[STIF_MAX_GROUPS];     /* packed, see stif_pack_conv_weight */
  const float* bias[STIF_MAX_GROUPS];  /* [cout_pad], packed order */
  float* out[STIF_MAX_GROUPS];
  const float* res[STIF_MAX_GROUPS];   /* STIF_EPI_RES: residual; STIF_EPI_LSTM: c_cur */
  float* out2[STIF_MAX_GROUPS];        /* STIF_EPI_LSTM: c_next */
  long long in0_item, in1_item, out_item, res_item, out2_item;  /* element strides between items */
  int ngroups, nitems;
  int H, W, C0;            /* in0: H x W x C0, C0 % 8 == 0 */
  int C1, in1_mode;        /* in1_mode: 0 none, 1 same resolution, 2 half resolution + x2 bilinear */
  float in1_scale;
  int Ho, Wo;              /* output resolution */
  int cout;                /* logical output channels (64, 216, 256) */
  int ks, stride;          /* 1 or 3; 1 or 2 (padding = ks/2) */
  int epi;                 /* STIF_EPI_* */
  int flags;               /* STIF_CONV_F16X3: weights packed with STIF_PACK_F16X3 (stif_conv3x3_wino only) */
  int* status;             /* optional device word (NULL = none): with STIF_CONV_F16X3, set to 1 when an output
                              element is not finite before its activation -- the signature of an activation
                              outside the split-fp16 operand range (see STIF_CONV_F16X3) */
  int* sched;              /* device block of 8 ints, zero when first used, read only with flags & STIF_CONV_DYNAMIC
                              (stif_conv3x3_wino, STIF_CONV_F16X3 launches; ignored otherwise, and ignored while the
                              stream is capturing a graph): per-XCD tile counters of the persistent kernel's dynamic
                              schedule.  The library keeps each block's running totals on the host, so the launches
                              that use one block must run in issue order (one stream) and the block must not be
                              freed and re-allocated while the library is loaded.  Outputs are identical either way.
                              Zero-initialise the whole struct: fields added at its end keep their old meaning
                              only when zero. */
  int item_base[STIF_MAX_GROUPS + 1];  /* per-set item counts as a prefix array; all zeros = `nitems` per set */
} stif_conv_args;

/* stif_conv_args.flags: fp32 products on the fp16 MFMA pipe by 3-term operand splitting (x = h + l,
 * a*b = ah*bh + ah*bl + al*bh, fp32 accumulation; ~22 significant bits per operand, see
 * stif_common.h).  Valid range: |activations| < 1024 (Winograd: |transformed inputs| < 4096),
 * |packed weights| < 64.  Both limits are enforced: the packers return STIF_E_RANGE for a weight
 * outside it, and an activation outside it turns the outputs it feeds into NaN/inf, which the
 * kernels report through the `status` word (the host then re-runs the call in fp32). */
#define STIF_CONV_F16X3 1
/* stif_conv_args.flags: take the persistent Winograd conv's tiles from the per-XCD counters in `sched`
 * (dynamic schedule) instead of the static stride; without this bit `sched` is never read. */
#define STIF_CONV_DYNAMIC 2

int stif_conv2d_nhwc(const stif_conv_args* args, void* stream);

/* The same operator for 3x3 / stride 1 / 'same' shapes by Winograd F(2x2,3x3) on fp32 MFMA
 * (2.25x fewer multiply-adds; all arithmetic fp32): weights packed with STIF_PACK_WINO
 * (epi NONE / LRELU / RELU / RES), STIF_PACK_WINO_OFFMASK (epi OFFMASK, cout 216) or
 * STIF_PACK_WINO_LSTM (epi LSTM, 128 -> 256: out = h_next, out2 = c_next, res = c_cur, 64-ch maps);
 * in1_mode 0 or 1; C0 and C1 multiples of 32. */
int stif_conv3x3_wino(const stif_conv_args* args, void* stream);

/* Weight and bias gradient of the 3x3 / stride 1 / 'same' convolution (training):
 *   gw[co][ci][kh][kw] = sum_{n,y,x} gy[n][y][x][co] * x[n][y + kh - 1][x + kw - 1][ci]  (zero outside the map),
 *   gb[co] = sum_{n,y,x} gy[n][y][x][co].
 * x (the forward's input) and gy (the gradient of its output) are NHWC fp32 maps of n items, x_item / gy_item
 * elements apart (>= 0, multiples of 4; bases 16-B aligned); gw is written in the state dict's OIHW order, gb may
 * be NULL; both are overwritten.  cin = cout = 64 only (the struct carries both so other shapes can follow).
 * Exact fp32 products on fp32 MFMA, fp32 accumulation.  No floating-point atomics: a persistent grid of G
 * workgroups (G a function of n, H, W and the device's CU count) takes the tiles in a static order, each writes
 * one partial sum to the workspace, and a second launch adds the G partials in index order, so repeated calls on
 * one device give identical bits.  workspace: at least stif_conv3x3_wgrad_workspace_size bytes, 16-B aligned;
 * its previous contents do not matter.  STIF_E_INVALID, each with its reason, before any launch: null args, a
 * null x / gy / gw, n / H / W < 1, other channel counts, a negative or misaligned stride, an item of 2 GB or more
 * (the limit stif_conv3x3_wino enforces), a workspace that is missing, too small or misaligned.
 * Zero-initialise the struct, then fill. */
typedef struct {
  const float* x;
  const float* gy;
  float* gw;               /* [cout][cin][3][3] */
  float* gb;               /* [cout] or NULL */
  long long x_item, gy_item;
  int n, H, W, cin, cout;
  void* workspace;
  size_t workspace_bytes;
} stif_conv_wgrad_args;
/* 0 for sizes < 1 or unsupported channel counts.  Pure host once the device's CU count is known. */
size_t stif_conv3x3_wgrad_workspace_size(int n, int H, int W, int cin, int cout);
int stif_conv3x3_wgrad(const stif_conv_wgrad_args* args, void* stream);

/* The same for the 3x3 / stride 2 / pad 1 convolution (the pyramid's fea_L*_conv1), same struct: H, W are the size
 * of x (the forward's input), gy is [n][Ho][Wo][64] with Ho = (H + 1) / 2, Wo = (W + 1) / 2, and
 *   gw[co][ci][kh][kw] = sum_{n,oy,ox} gy[n][oy][ox][co] * x[n][2 oy + kh - 1][2 ox + kw - 1][ci]  (zero outside).
 * Same partial-sum scheme, determinism contract, workspace rules and rejections as stif_conv3x3_wgrad. */
size_t stif_conv3x3s2_wgrad_workspace_size(int n, int H, int W, int cin, int cout);
int stif_conv3x3s2_wgrad(const stif_conv_wgrad_args* args, void* stream);

/* Data gradient of the 3x3 / stride 2 / pad 1 / 64 -> 64 convolution (a transposed conv):
 *   gx[n][y][x][ci] = sum over (kh, kw, co) with y + 1 - kh and x + 1 - kw even and (oy, ox) = ((y + 1 - kh) / 2,
 *   (x + 1 - kw) / 2) inside [0, Ho) x [0, Wo) of gy[n][oy][ox][co] * w[co][ci][kh][kw].
 * gy [n][Ho][Wo][64] and gx [n][H][W][64] are NHWC fp32 maps, gy_item / gx_item elements apart (>= 0, multiples of 4;
 * bases 16-B aligned); H, W (the forward input's size) are given because Ho does not determine them.  w_oihw is the
 * state dict's weight on the device (transposed by the kernel's own loads: the workspace size is 0 and workspace may
 * be NULL).  gx is overwritten in full, each element by one lane; exact fp32 products on fp32 MFMA, split by the
 * parity of the gx pixel so that no multiply-add is spent on an inserted zero.  STIF_E_INVALID before any launch:
 * a null gy / w_oihw / gx, n / H / W < 1, a negative or misaligned stride, an item of 2 GB or more. */
size_t stif_conv3x3s2_dgrad_workspace_size(int n, int H, int W);
int stif_conv3x3s2_dgrad(const float* gy, const float* w_oihw, float* gx, long long gy_item, long long gx_item,
                         int n, int H, int W, void* workspace, size_t workspace_bytes, void* stream);

/* Weight and bias gradient of conv_first (3 -> 64, 3x3 'same'): x_nchw the RGB frames [n,3,h,w] as stif_conv_first
 * reads them, gy NHWC [n][h][w][64] (items gy_item elements apart, >= 0, a multiple of 4; base 16-B aligned),
 * gw [64][3][3][3], gb [64] or NULL.  Two launches -- per-workgroup partials into the workspace, then a reduce in
 * index order -- so repeated calls on one device give identical bits; the workspace (at least
 * stif_conv_first_wgrad_workspace_size bytes, 16-B aligned) may hold anything.  The gradient with respect to the
 * frames is not computed.  STIF_E_INVALID before any launch as for stif_conv3x3_wgrad. */
size_t stif_conv_first_wgrad_workspace_size(int n, int h, int w);
int stif_conv_first_wgrad(const float* x_nchw, const float* gy, float* gw, float* gb, long long gy_item,
                          int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* The weight and bias gradient of stif_conv3x3_wgrad in 64 x 64 channel blocks, for the 3x3 'same' convs of PCD_Align
 * whose input or output is wider than 64 channels (training):
 *   gw[co][64 i + ci][kh][kw] = sum_{n,y,x} gy[n][y][x][co] * x[i][n][y + kh - 1][x + kw - 1][ci],  co < cout,
 *   gb[co] = sum_{n,y,x} gy[n][y][x][co].
 * x[0], x[1]: the halves of the forward's concatenated input (nx = 2; the concatenation is never built), NHWC
 * 64-channel maps; gy: NHWC with a pixel pitch of gy_channels floats of which the first cout count (the rest is never read).
 * Supported (nx, gy_channels, cout): (2, 64, 64) the 128 -> 64 concatenation convs, (1, 256, 216) conv_offset_mask
 * with its gradient in the zero-padded 256-channel map the Winograd conv writes, (1, 64, 64) = stif_conv3x3_wgrad,
 * (2, 256, 256) the ConvLSTM cell's 128 -> 256 conv on (input | hidden state), eight blocks.
 * One launch computes every block (cout slice, x map) as stif_conv3x3_wgrad's walk over the same tiles with the same
 * grid, one partial per workgroup and block, and a second adds each block's partials in index order: no
 * floating-point atomics, identical bits for repeated calls, and every 64 x 64 block of gw equals
 * stif_conv3x3_wgrad's result for the same two 64-channel maps.  workspace: at least
 * stif_conv3x3_wgrad_cat_workspace_size bytes (blocks x stif_conv3x3_wgrad_workspace_size), 16-B aligned.
 * STIF_E_INVALID, each with its reason, before any launch: null args, a null x[0] / gy / gw, nx = 2 with a null x[1],
 * n / H / W < 1, other channel counts, a negative or misaligned stride or base, an item of 2 GB or more (H W
 * gy_channels floats), a workspace that is missing, too small or misaligned.  Zero-initialise the struct, then fill. */
typedef struct {
  const float* x[2];       /* the halves of the forward's concatenated input, NHWC [n][H][W][64] each */
  const float* gy;         /* NHWC [n][H][W][gy_channels] */
  float* gw;               /* [cout][64 * nx][3][3], OIHW as the state dict has it */
  float* gb;               /* [cout] or NULL */
  long long x_item[2], gy_item;
  int n, H, W;
  int nx;                  /* 1 or 2 */
  int gy_channels, cout;   /* (64, 64), (256, 216) or (256, 256): the pixel pitch of gy and the channels that count */
  void* workspace;
  size_t workspace_bytes;
} stif_conv_wgrad_cat_args;
/* 0 for sizes < 1 or unsupported channel counts. */
size_t stif_conv3x3_wgrad_cat_workspace_size(int n, int H, int W, int nx, int gy_channels, int cout);
int stif_conv3x3_wgrad_cat(const stif_conv_wgrad_cat_args* args, void* stream);

/* The weight and bias gradient of the 1x1 conv on one or two 64-channel inputs (fusion, Easy_PCD.fusion,
 * ConvBLSTM.conv_1x1: (64 | 64) -> 64; nx = 1 is the 64 -> 64 form), training:
 *   gw[co][64 i + ci] = sum_{n,y,x} gy[n][y][x][co] * x[i][n][y][x][ci],   gb[co] = sum_{n,y,x} gy[n][y][x][co].
 * The arguments are stif_conv_wgrad_cat_args with gy_channels = cout = 64; gw is [64][64 nx][1][1] OIHW.  fp32 MFMA,
 * and the deterministic scheme of stif_conv3x3_wgrad: the grid is a function of the shape and the CU count, every
 * workgroup writes one partial, a second kernel adds them in an order fixed by their number (sixteen interleaved
 * index-ordered slices, then the slices in order: no atomics, identical bits for repeated calls); the workspace (stif_conv1x1_wgrad_workspace_size bytes, 0 for sizes < 1 or nx outside {1, 2}; 16-B aligned)
 * may hold anything on entry.  STIF_E_INVALID before any launch as for stif_conv3x3_wgrad_cat. */
size_t stif_conv1x1_wgrad_workspace_size(int n, int H, int W, int nx);
int stif_conv1x1_wgrad(const stif_conv_wgrad_cat_args* args, void* stream);

/* The ConvLSTM cell's gates (convlstm.py:44-57) on the pre-activations of its 128 -> 256 conv, for training: pre
 * [n][H][W][256] in the reference's row order (channel gate * 64 + h, gates i, f, o, g: what stif_conv3x3_wino writes
 * with STIF_EPI_NONE from a STIF_PACK_WINO pack of the weight), c_cur / h_next / c_next [n][H][W][64]:
 *   c_next = sigmoid(f) c_cur + sigmoid(i) tanh(g),   h_next = sigmoid(o) tanh(c_next).
 * Items *_item floats apart (>= 0, multiples of 4; bases 16-B aligned; pixels contiguous); finite for any finite
 * pre-activation.  STIF_E_INVALID before the launch: a null pointer, n / H / W < 1, a negative or misaligned stride or
 * base, an item of 2 GB or more (H W 256 floats), output items that overlap. */
int stif_lstm_gates_nhwc(const float* pre, const float* c_cur, float* h_next, float* c_next, int n, int H, int W,
                         long long pre_item, long long c_item, long long h_item, long long cn_item, void* stream);
/* Its backward.  The forward saves only pre and c_cur; the gates and tanh(c_next) are recomputed.  With
 * dc = g_c_next + g_h o (1 - tanh^2 c_next):  g_pre_i = dc g i (1 - i), g_pre_f = dc c_cur f (1 - f),
 * g_pre_o = g_h tanh(c_next) o (1 - o), g_pre_g = dc i (1 - g^2), g_c_cur = dc f.  g_h or g_c_next may be NULL (zeros;
 * both NULL is STIF_E_INVALID), g_c_cur may be NULL (not computed); g_pre [n][H][W][256].  Checks as the forward's. */
int stif_lstm_gates_bwd_nhwc(const float* pre, const float* c_cur, const float* g_h, const float* g_c_next,
                             float* g_pre, float* g_c_cur, int n, int H, int W, long long pre_item, long long c_item,
                             long long gh_item, long long gcn_item, long long gpre_item, long long gcc_item,
                             void* stream);

/* The adjoint of stif_upsample2x_nhwc: gx = the transpose of scale * F.interpolate(scale_factor=2, bilinear,
 * align_corners=False) applied to gy [n][2 h1][2 w1][c]; gx [n][h1][w1][c], c % 4 == 0, items gy_item / gx_item floats
 * apart (>= 0, multiples of 4; bases 16-B aligned).  Gather form: every gx element is written once, by one lane, from a
 * 4 x 4 window of gy in a fixed addition order (no atomics); h1 = 1 and w1 = 1 are served. */
int stif_upsample2x_bwd_nhwc(const float* gy, float* gx, int n, int h1, int w1, int c, float scale,
                             long long gy_item, long long gx_item, void* stream);

/* out = scale * F.interpolate(in, scale_factor=2, mode='bilinear', align_corners=False) on NHWC
 * maps (PCD_Align's coarse-to-fine step, Sakuya_arch_test.py:86-87); in [n][h1][w1][c],
 * out [n][2h1][2w1][c], items `in_item` / `out_item` floats apart, c % 4 == 0. */
int stif_upsample2x_nhwc(const float* in, float* out, int n, int h1, int w1, int c, float scale,
                         long long in_item, long long out_item, void* stream);

/* ---- the SIREN decoder for training ----
 *
 * The three MLPs (feat_imnet, flow_imnet, encode_imnet; SIREN.py:74-79) run on input matrices in HBM, row-major fp32,
 * one row per HR pixel: x [n][x_stride], of which the first cin columns are the inputs (201, 263 or 525) and columns
 * cin .. round8(cin) - 1 are zeros; x_stride is a multiple of 8, at least round8(cin) (columns past round8(cin) are
 * never read).  nsine sine layers of widths width[0 .. nsine) -- (64, 64, 256) or (64, 64, 256, 256), width[3] = 0 with
 * three -- each sin(30 (a W^T + b)), then a linear layer to cout in {64, 4, 3}.  w[l] / b[l]: the parameter tensors,
 * row-major [cout_l][cin_l] and [cout_l] (the last at index nsine).  fp32 MFMA, exact fp32 products.
 *
 * stif_siren_fwd writes y [n][cout] and z [n][zw], zw = 384 or 640: the pre-activations z_l = a_{l-1} W_l^T + b_l of
 * the sine layers side by side (layer l at column width[0] + .. + width[l - 1]).  No activation is stored.
 *
 * stif_siren_bwd takes g_y [n][cout], x and the z of the forward, and writes g_w[l] / g_b[l] (the shapes of w / b) of
 * every layer and, unless g_x is NULL, g_x [n][gx_stride] (gx_stride as x_stride): columns < cin the input gradient,
 * cin .. round8(cin) - 1 zeros.  sin and cos are recomputed from z.  The weight and bias gradients use no atomics:
 * per layer, workgroups write partial sums of 64 x 64 blocks into the workspace and a second launch adds them in an
 * order fixed by their number, stif_siren_wgrad_grid(n, cout_l, cin_l) per block -- a function of n, the layer's shape
 * and the CU count (0 for sizes out of range).  Repeated calls give identical bits whatever the workspace held.
 * workspace: stif_siren_bwd_workspace_size(n, nsine) bytes (0 for n < 1 or nsine outside {3, 4}), 16-B aligned; it
 * holds the g_z of every sine layer (n zw floats) and the partials.
 *
 * STIF_E_INVALID, each with its reason, before any launch: null args, a null x / z / y / w[l] / b[l] (backward: g_y,
 * g_w[l], g_b[l], workspace), n < 1, nsine or widths other than the two lists, cout outside {64, 4, 3}, cin outside
 * [1, STIF_SIREN_MAX_CIN], a stride that is not a multiple of 8 or smaller than round8(cin), x / z / g_x / workspace
 * not 16-B aligned, a workspace that is too small.  Zero-initialise the struct, then fill. */
#define STIF_SIREN_ROW_TILE 64   /* rows per workgroup of the MLP kernels */
#define STIF_SIREN_MAX_CIN 528
typedef struct {
  const float* x;
  long long x_stride;
  int n, cin, nsine, cout;
  int width[4];
  const float* w[5];
  const float* b[5];
  float* y;                /* forward: [n][cout] */
  float* z;                /* [n][zw]: written by the forward, read by the backward */
  const float* g_y;        /* backward: [n][cout] */
  float* g_x;              /* backward: [n][gx_stride] or NULL */
  long long gx_stride;
  float* g_w[5];
  float* g_b[5];
  void* workspace;
  size_t workspace_bytes;
} stif_siren_args;
int stif_siren_fwd(const stif_siren_args* args, void* stream);
size_t stif_siren_bwd_workspace_size(int n, int nsine);
int stif_siren_wgrad_grid(int n, int cout, int cin);
int stif_siren_bwd(const stif_siren_args* args, void* stream);

/* The builders of the three MLP input matrices and their adjoints (Sakuya_arch_test.py:364-459 without the local
 * ensemble; N = B HH WW rows, pixel (b, qy, qx) at row (b HH + qy) WW + qx):
 *   X1 [N][208]: latent at the nearest LR pixel 192 | frames there 6 | rel_y, rel_x | t | 7 zeros;
 *   X2 [N][264]: HRfeat 64 | bilinear latent 192 | bilinear frames 6 | t | 1 zero  (the fixed query grid);
 *   X3 [N][528]: HRfeat@grid1 64 | HRfeat@grid2 64 | latent@grid1 192 | latent@grid2 192 | frames@grid1 6 |
 *                frames@grid2 6 | t | 3 zeros, the grids torch.linspace + flow / ((n - 1) / 2) clamped to
 *                +-(1 - 1e-6), flow [N][4] = (x1, y1, x2, y2) in HR pixels; bilinear with zero padding.
 * feat [B][H][W][192] is the NHWC latent, frames [B][6][H][W] the planar LR frame pair, t [B] a time per item,
 * hrfeat [N][64].  The per-row / per-column tables are the host's (coords.dec_tables: HH / WW entries), the *_first
 * tables their inverses for the gather-form adjoints (H + 1 / W + 1 entries: the first HR index whose table entry is
 * >= i; every table is monotone).
 * Adjoints: x1_bwd writes g_feat [B][H][W][192], each element the sum of the g_X1 rows of the HR rectangle whose
 * nearest pixel it is; x2_bwd writes g_hrfeat [N][64] = g_X2[:, :64] and g_feat, the adjoint of the fixed bilinear
 * gather (both gather form, one lane per element in a fixed order: identical bits for repeated calls).  x3_bwd
 * writes g_flow [N][4] with plain stores (the coordinate gradient of all six samples; exactly zero where the clamp is
 * active) and ADDS into g_hrfeat [N][64] and g_feat, which the caller zeroes, with fp32 atomics on whole channel rows:
 * the only order-dependent sums of the decoder backward (stif_dec_x3_bwd_contrib + stif_segsum, below, is the ordered
 * alternative with identical bits on every run).  No gradient goes to frames or t.
 * STIF_E_INVALID before any launch: null geometry, a null pointer in it or among the arguments, B / H / W < 1,
 * HH / WW < 2 (the warp grid divides by n - 1), more than 2^31 - 1 float4 of any matrix. */
typedef struct {
  int B, H, W, HH, WW;
  const float* feat;
  const float* frames;
  const float* t;
  const int *near_y, *near_x;
  const float *rel_y, *rel_x;
  const int *by0, *by1, *bx0, *bx1;
  const float *wy0, *wy1, *wx0, *wx1;
  const float *lin_y, *lin_x;
  const int *near_y_first, *near_x_first, *by0_first, *by1_first, *bx0_first, *bx1_first;
} stif_dec_train_geom;
int stif_dec_x1_fwd(const stif_dec_train_geom* g, float* x1, void* stream);
int stif_dec_x1_bwd(const stif_dec_train_geom* g, const float* g_x1, float* g_feat, void* stream);
int stif_dec_x2_fwd(const stif_dec_train_geom* g, const float* hrfeat, float* x2, void* stream);
int stif_dec_x2_bwd(const stif_dec_train_geom* g, const float* g_x2, float* g_hrfeat, float* g_feat, void* stream);
int stif_dec_x3_fwd(const stif_dec_train_geom* g, const float* hrfeat, const float* flow, float* x3, void* stream);
int stif_dec_x3_bwd(const stif_dec_train_geom* g, const float* hrfeat, const float* flow, const float* g_x3,
                    float* g_flow, float* g_hrfeat, float* g_feat, void* stream);

/* conv_first (3 -> 64, 3x3) + LeakyReLU, reading NCHW RGB frames [n,3,h,w]
 * (Sakuya_arch_test.py:318) and writing NHWC [n,h,w,64]. w: [64,3,3,3] as in the state dict. */
int stif_conv_first(const float* x_nchw, const float* w, const float* b, float* out,
                    int n, int h, int w_, void* stream);

/* Fused modulated deformable conv (DCN_sep core, 64 -> 64, 3x3, 8 groups):
 * bilinear sampling (dmcn_im2col_bilinear semantics) straight into LDS and an
 * fp32-MFMA contraction; no columns buffer.  offmask is the NHWC output of the
 * offset/mask conv packed with STIF_PACK_OFFMASK (216 channels per pixel,
 * [group][tap][dy, dx, sigmoid(mask)]). */
typedef struct {
  const float* in[STIF_MAX_GROUPS];
  const float* offmask[STIF_MAX_GROUPS];
  const float* w[STIF_MAX_GROUPS];     /* packed like a 64->64 3x3 conv */
  const float* bias[STIF_MAX_GROUPS];
  float* out[STIF_MAX_GROUPS];
  long long in_item, om_item, out_item;
  int ngroups, nitems, H, W;
  int epi;                              /* STIF_EPI_NONE or STIF_EPI_LRELU */
  int flags;                            /* STIF_CONV_F16X3: w packed STIF_PACK_PLAIN | STIF_PACK_F16X3 */
  int* status;                          /* optional device word, as stif_conv_args.status */
  int item_base[STIF_MAX_GROUPS + 1];   /* per-set item counts as a prefix array; all zeros = `nitems` per set */
} stif_dcn_args;

int stif_dcn_nhwc(const stif_dcn_args* args, void* stream);

/* Backward of stif_dcn_nhwc (one group, fp32) at the same shape, NHWC throughout (training; the formulas are
 * modulated_deformable_col2im / _col2im_coord and dcn_v2_cuda_backward's weight / bias gradient).  With
 *   gy = gout, or with epi = STIF_EPI_LRELU gout * (out > 0 ? 1 : 0.1)   (the activation's derivative from its output),
 *   colg[p][c][k] = sum_co w[co][c][k] * gy[p][co],
 *   g_in   += colg * m * bilinear weight at the four corners of every sample (corners outside the frame get nothing),
 *   g_w[co][c][k] = sum_p gy[p][co] * m * sample(p, c, k),   g_b[co] = sum_p gy[p][co],
 * and g_om in the layout of the offset / mask conv's 256-channel output map, so that it is that conv's output
 * gradient as it stands: channel g*18 + 2k (+1) = grad_offset h (w) of group g, tap k; channel 144 + g*9 + k =
 * grad_mask * m * (1 - m) with m read from offmask (the sigmoid's derivative); channels 216..255 zeros.
 * All pointers are device pointers, bases 16-B aligned, items *_item floats apart (>= 0, multiples of 4; the items of
 * g_in / g_om must not overlap); nothing is read back and nothing is allocated.  A NULL output is not computed: the
 * weight kernel runs only with g_w, the data kernel only with g_in or g_om.  Every output asked for is overwritten
 * in full; g_in is cleared on `stream` first.  g_om, g_w and g_b are written without floating-point atomics, each
 * element by one lane (g_w / g_b through per-workgroup partials in the workspace, added in index order as
 * stif_conv3x3_wgrad does), so repeated calls on one device give identical bits for these three.  g_in is a sum of
 * fp32 atomic adds -- as in the reference and the drop-in -- whose order varies: its last bits may differ from run to
 * run; the ordered alternative, with identical bits on every run, is stif_dcn_bwd_contrib + a sort of its packed
 * words + stif_segsum (below).  workspace (needed with g_w only): at least stif_dcn_bwd_workspace_size bytes, which equals
 * stif_conv3x3_wgrad_workspace_size(n, H, W, 64, 64), 16-B aligned; its previous contents do not matter.
 * STIF_E_INVALID, each with its reason, before any launch: null args, a null in / offmask / w / gout, an unknown epi,
 * epi LRELU with a null out, all of g_in / g_om / g_w null, g_b without g_w, n / H / W < 1, a negative or misaligned
 * stride or base, overlapping g_in / g_om items, an item of 2 GB or more (H W 256 floats), and with g_w a workspace
 * that is missing, too small or misaligned.  Zero-initialise the struct, then fill. */
typedef struct {
  const float* in;       /* the forward's input, NHWC [n][H][W][64] */
  const float* offmask;  /* what stif_dcn_nhwc read: NHWC [n][H][W][216] = [group 8][tap 9][dy, dx, m], m after the sigmoid */
  const float* w;        /* the state dict's weight [64][64][3][3] on the device (no host packing, no sync) */
  const float* gout;     /* gradient of the forward's output, NHWC [n][H][W][64] */
  const float* out;      /* the forward's output, NHWC; read only with epi = STIF_EPI_LRELU */
  float* g_in;           /* NHWC [n][H][W][64], or NULL: not computed */
  float* g_om;           /* NHWC [n][H][W][256], or NULL: not computed */
  float* g_w;            /* [64][64][3][3] OIHW, or NULL: neither g_w nor g_b computed */
  float* g_b;            /* [64] or NULL */
  long long in_item, om_item, gout_item, out_item, gin_item, gom_item;
  int n, H, W;
  int epi;               /* STIF_EPI_NONE, or STIF_EPI_LRELU: gout is first multiplied by 0.1 where out <= 0 */
  void* workspace;
  size_t workspace_bytes;
} stif_dcn_bwd_args;
/* 0 for sizes < 1. */
size_t stif_dcn_bwd_workspace_size(int n, int H, int W);
int stif_dcn_bwd_nhwc(const stif_dcn_bwd_args* args, void* stream);

/* ---- Deterministic training: ordered sums in place of the three atomic scatters (g_in of stif_dcn_bwd_nhwc, g_hrfeat
 * and g_feat of stif_dec_x3_bwd).  Every contribution is stored once with plain stores, the caller sorts the packed
 * words (any stable or unstable sort: the words are unique), and stif_segsum adds per destination in a fixed order.
 *
 * A scatter is a list of E entries e = 0 .. E-1.  Entry e has a destination row key[e] in 0 .. D (D: "this corner does
 * not count"), an fp32 weight w[e], and a source sub-row of C floats at
 *   src + ((e >> 2) / K) * row_stride + ((e >> 2) % K) * C + col0
 * (four corners share a sub-row).  Its packed word is (key[e] << 32) | e as int64.  The value of dst[d][c], d < D:
 * take the entries with key[e] == d in ascending e, cut the list into chunks of 512, within a chunk start from +0.0f
 * and do acc = acc + (w[e] * src_e[c]) -- an fp32 multiply and an fp32 add, both rounded to nearest, NOT fused -- and
 * add the chunk partials the same way in chunk order, starting from the first partial.  A list of at most 512 entries
 * is a plain sequential sum; an empty list gives +0.0f.
 *
 * stif_segsum: dst [D][C] (every row overwritten), `sorted` the packed words in ascending order, seg [D + 1] with
 * seg[d] = the index in `sorted` of the first word whose key is >= d.  C is 8, 64 or 192.  The kernel does not trust
 * the indices: segment bounds are clamped to [0, E], an entry id >= E is skipped, every loop is bounded by E; src
 * must hold ceil(E / 4 / K) rows of row_stride floats and w E floats.  No floating-point atomics; repeated calls give
 * identical bits.  STIF_E_INVALID before the launch: a null pointer, C not 8 / 64 / 192, D / E / K < 1, D or E >= 2^31,
 * col0 < 0, col0 or row_stride no multiple of 4, row_stride < K * C + col0, dst / src not 16-byte, w not 4-byte,
 * sorted / seg not 8-byte aligned. */
int stif_segsum(float* dst, const float* src, long long row_stride, int K, int col0, const float* w,
                const long long* sorted, const long long* seg, long long D, long long E, int C, void* stream);

/* stif_dcn_bwd_nhwc's data kernel with stores in place of the g_in scatter (the same MFMA front end): g_om exactly as
 * stif_dcn_bwd_nhwc writes it (same bytes; NULL: not written), and for pixel p = (i H + y) W + x of the call, group g,
 * tap k, corner j (low/low, low/high, high/low, high/high), e = ((p * 8 + g) * 9 + k) * 4 + j:
 *   cm [n H W][8][9][8]  the contribution sub-rows colg * m, every one written (zeros where no corner counts),
 *   wgt [E]              the corner's bilinear weight product (0 for a corner that does not count),
 *   words [E]            (key << 32) | e, key = (pixel index of the corner) * 8 + g, or D = n H W 8.
 * E = n H W 288.  g_in [n][H][W][64] dense is then stif_segsum(g_in, cm, 576, 72, 0, wgt, sorted words, seg, D, E, 8).
 * Inputs and strides as stif_dcn_bwd_args; all buffers are the caller's, nothing is allocated.  STIF_E_INVALID before
 * the launch: null args, a null in / offmask / w / gout / cm / wgt / words, an unknown epi, epi LRELU with a null out,
 * n / H / W < 1, a negative or misaligned stride or base (16 bytes), overlapping g_om items, an item of 2 GB or more,
 * E >= 2^31 (call it on fewer items: items are independent).  Zero-initialise the struct, then fill. */
typedef struct {
  const float* in;
  const float* offmask;
  const float* w;
  const float* gout;
  const float* out;      /* read only with epi = STIF_EPI_LRELU */
  float* g_om;           /* NHWC [n][H][W][256], or NULL */
  float* cm;
  float* wgt;
  long long* words;
  long long in_item, om_item, gout_item, out_item, gom_item;
  int n, H, W;
  int epi;
} stif_dcn_bwd_contrib_args;
int stif_dcn_bwd_contrib(const stif_dcn_bwd_contrib_args* args, void* stream);

/* stif_dec_x3_bwd with stores in place of its two scatters: g_flow exactly as stif_dec_x3_bwd writes it (same bytes),
 * and for HR pixel row n of g_x3, grid k (0, 1), corner j (y0 x0, y0 x1, y1 x0, y1 x1), e = (n * 2 + k) * 4 + j, the
 * weight wx * wy (0 outside the map) and the packed word of the corner on the HR lattice (w_hr, words_hr: key =
 * b HH WW + y WW + x, or D = B HH WW) and on the LR lattice (w_lr, words_lr: key = b H W + y W + x, or D = B H W).
 * E = 8 N.  The source sub-rows are g_x3 itself:
 *   g_hrfeat = stif_segsum(.., g_x3, 528, 2, 0, w_hr, .., D = N, E, 64),
 *   g_feat   = stif_segsum(.., g_x3, 528, 2, 128, w_lr, .., D = B H W, E, 192).
 * STIF_E_INVALID as stif_dec_x3_bwd, and: a null w_hr / words_hr / w_lr / words_lr, words not 8-byte aligned,
 * E >= 2^31. */
int stif_dec_x3_bwd_contrib(const stif_dec_train_geom* g, const float* hrfeat, const float* flow, const float* g_x3,
                            float* g_flow, float* w_hr, long long* words_hr, float* w_lr, long long* words_lr,
                            void* stream);

/* ---- Data-parallel training: the gradient arena and the rank-ordered sum.
 *
 * stif_grad_pack gathers nseg fp32 tensors into one arena in a single launch.  segs_dev is a device table of nseg
 * stif_grad_seg in ascending dst order: segment s copies n floats from src (4-byte aligned; 16-byte loads where the
 * address allows, dword loads otherwise) to arena + dst, dst a multiple of 4 floats.  The gap after a segment up to the
 * next multiple of 4 and the arena's tail -- from the end of the last segment, rounded up to 4, to arena_floats -- are
 * written as +0.0f; floats between two segments beyond that gap are left as they are.  Stores are 16 bytes.
 * Workgroups walk chunks of STIF_GRAD_CHUNK floats: a segment has ceil(n / STIF_GRAD_CHUNK) chunks (none for n = 0),
 * a chunk never spans segments, and chunk0 is the prefix table, the number of chunks of the segments before this one.
 * The table's contents are the caller's responsibility; the kernel still bounds every access to the arena by
 * arena_floats, and its loops by nseg and arena_floats.  STIF_E_INVALID before the launch: a null pointer, nseg < 1 or
 * above STIF_GRAD_MAX_SEGS, an arena that is not 16-byte or a table that is not 8-byte aligned, arena_floats < 4, not
 * a multiple of 4 or above 2^31 - 1. */
#define STIF_GRAD_CHUNK 1024
#define STIF_GRAD_MAX_SEGS (1 << 20)
typedef struct {
  const float* src;
  long long dst;       /* offset in the arena, in floats */
  long long n;         /* floats */
  long long chunk0;    /* chunks of the segments before this one */
} stif_grad_seg;
int stif_grad_pack(const stif_grad_seg* segs_dev, int nseg, float* arena, long long arena_floats, void* stream);

/* dst[i] = ((slab[0][i] + slab[1][i]) + ...) + slab[R - 1][i] for i < n, slab[r] = slab + r * row_floats: plain fp32
 * adds, rounded to nearest, in rank order; R = 1 copies.  No atomics and nothing to contract: repeated calls give
 * identical bits, whatever the grid.  STIF_E_INVALID before the launch: a null pointer, R outside 1 ..
 * STIF_RANK_SUM_MAX_RANKS, n < 4 or not a multiple of 4, n > row_floats, row_floats not a multiple of 4, n or
 * row_floats above 2^31 - 1, slab or dst not 16-byte aligned, dst overlapping the R rows read. */
#define STIF_RANK_SUM_MAX_RANKS 64
int stif_rank_sum(const float* slab, long long row_floats, int R, float* dst, long long n, void* stream);

/* The offset / mask conv's output as the deformable conv reads it: om NHWC [n][H][W][256] in the reference's row order
 * (channel g*18 + 2k (+1) the h (w) offset of group g, tap k; 144 + g*9 + k the mask logit; 216..255 never read) ->
 * offmask NHWC [n][H][W][216] = [group][tap][dy, dx, sigmoid(logit)].  Offsets are copied bit for bit; the sigmoid is
 * 1 / (1 + expf(-x)).  Items om_item / offmask_item floats apart (>= 0, multiples of 4; bases 16-B aligned; offmask
 * items must not overlap).  STIF_E_INVALID before the launch: a null om / offmask, n / H / W < 1, a negative or
 * misaligned stride or base, overlapping offmask items, an item of 2 GB or more (H W 256 floats). */
int stif_dcn_offmask_nhwc(const float* om, float* offmask, long long om_item, long long offmask_item, int n, int H,
                          int W, void* stream);

/* Fused DCN_sep (dcn_v2.py:127-140) in one launch: conv_offset_mask (64 -> 216, 3x3) + chunk / cat /
 * sigmoid + the modulated deformable conv (64 -> 64, 3x3, 8 groups) -- the offset/mask map never leaves
 * the registers (split-fp16 MFMA only, flags = STIF_CONV_F16X3).  fea: the offset branch's feature
 * (NHWC 64 ch); in: the deformable conv's input (NHWC 64 ch); w_om / b_om: conv_offset_mask packed
 * with STIF_PACK_DCNSEP | STIF_PACK_F16X3; w / bias: the DCN weight packed STIF_PACK_DCNPAIR |
 * STIF_PACK_F16X3.  Replaces the pair conv (STIF_EPI_OFFMASK) -> stif_dcn_nhwc. */
typedef struct {
  const float* fea[STIF_MAX_GROUPS];
  const float* in[STIF_MAX_GROUPS];
  const float* w_om[STIF_MAX_GROUPS];
  const float* b_om[STIF_MAX_GROUPS];
  const float* w[STIF_MAX_GROUPS];
  const float* bias[STIF_MAX_GROUPS];
  float* out[STIF_MAX_GROUPS];
  long long fea_item, in_item, out_item;
  int ngroups, nitems, H, W;
  int epi;                              /* STIF_EPI_NONE or STIF_EPI_LRELU */
  int flags;                            /* STIF_CONV_F16X3 (required) */
  int* status;                          /* optional device word, as stif_conv_args.status */
  int item_base[STIF_MAX_GROUPS + 1];   /* per-set item counts as a prefix array; all zeros = `nitems` per set */
} stif_dcn_sep_args;

int stif_dcn_sep_nhwc(const stif_dcn_sep_args* args, void* stream);

/* Drop-in for `_ext.dcn_v2_forward` (dcn_v2.h:9-23): NCHW fp32 input [b,c,h,w],
 * weight [co,c,kh,kw], bias [co], offset [b, dg*2*kh*kw, ho, wo],
 * mask [b, dg*kh*kw, ho, wo]; output [b, co, ho, wo] (caller-allocated).
 * Any kernel/stride/pad/dilation/group combination of the reference is
 * accepted.  The STIF shape (c = co = 64, 3x3, stride 1, pad 1, dilation 1, 8 groups: every
 * DCN_sep of LunaTokis) runs the fused im2col-free kernel of stif_dcn_nhwc (fp32 MFMA) between
 * NCHW<->NHWC transposes, with the weights packed on the device -- workspace 344 floats per
 * pixel (the reference's im2col path: 576); every other shape runs im2col + GEMM one sample at a
 * time (workspace c*kh*kw*ho*wo floats, the reference's per-sample `columns`).
 * workspace: at least stif_dcn_v2_workspace_size bytes, 16-B aligned. */
size_t stif_dcn_v2_workspace_size(int batch, int channels, int height, int width, int channels_out,
                                  int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                  int pad_w, int dilation_h, int dilation_w, int deformable_group);
int stif_dcn_v2_forward(const float* input, const float* weight, const float* bias,
                        const float* offset, const float* mask, float* output,
                        int batch, int channels, int height, int width, int channels_out,
                        int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w,
                        int dilation_h, int dilation_w, int deformable_group,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Drop-in for `_ext.dcn_v2_backward` (dcn_v2.h:39-52, vision.cpp:5; CUDA body dcn_v2_cuda.cu:204-335):
 * the same NCHW tensors as stif_dcn_v2_forward plus grad_output [b, co, ho, wo]; writes grad_input
 * [b,c,h,w], grad_offset [b, dg*2*kh*kw, ho, wo], grad_mask [b, dg*kh*kw, ho, wo], grad_weight
 * [co,c,kh,kw] and grad_bias [co] (caller-allocated; all overwritten).  Per sample, as the reference:
 * columns gradient = W^T grad_output (fp32 MFMA GEMM), the coordinate / mask gradients
 * (modulated_deformable_col2im_coord semantics, one thread per group x tap x pixel), the input
 * gradient scattered to the bilinear corners with fp32 atomics (modulated_deformable_col2im), the
 * forward columns and grad_weight += grad_output columns^T, grad_bias += sum grad_output.
 * workspace: at least stif_dcn_v2_backward_workspace_size bytes (c*kh*kw*ho*wo floats), 16-B aligned. */
size_t stif_dcn_v2_backward_workspace_size(int batch, int channels, int height, int width, int channels_out,
                                           int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                           int pad_w, int dilation_h, int dilation_w, int deformable_group);
int stif_dcn_v2_backward(const float* input, const float* weight, const float* bias, const float* offset,
                         const float* mask, const float* grad_output, float* grad_input, float* grad_offset,
                         float* grad_mask, float* grad_weight, float* grad_bias, int batch, int channels, int height,
                         int width, int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w,
                         int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- implicit decoder (LunaTokis.decoding, Sakuya_arch_test.py:364-459) ---- */

/* Assemble the decoder's LR source map [n,h,w,200] = [feat t0 | t1 | t2 | inp rgb0 rgb1 | 0 0]
 * from the three NHWC latent maps and the NCHW input pair x [n,2,3,h,w]. */
int stif_dec_pack_lr(const float* f0, const float* f1, const float* f2, const float* x_nchw,
                     float* out, int n, int h, int w, void* stream);

/* Per-axis sampling tables of the HR query grid (host-computed, fp32, see
 * stif_amd.coords): for every HR row (then column): nearest LR index, rel
 * coordinate, bilinear LR indices i0/i1, weights w0/w1 (0 if out of range), and
 * the warpgrid linspace base. Layout: struct of arrays, one float/int per entry. */
typedef struct {
  const int* near_y; const float* rel_y; const int* by0; const int* by1; const float* wy0; const float* wy1;
  const float* lin_y;
  const int* near_x; const float* rel_x; const int* bx0; const int* bx1; const float* wx0; const float* wx1;
  const float* lin_x;
  /* optional (NULL = identity): HR pixel whose HRfeat the flow stage reads for a query -- the
   * local ensemble's shifted queries (decoding_localensemble, Sakuya_arch_test.py:1022-1025) */
  const int* hr_y; const int* hr_x;
} stif_dec_tables;

/* Optional high-resolution image for the flow / encode stages (decoding_test samples
 * HRinp = F.upsample(inp, x4, bilinear), Sakuya_arch_test.py:513-514, instead of the LR frames;
 * pack the projection with stif_pack_dec_proj_ex(..., lr_image = 0) then).  img: [n][ih][iw][8]
 * (rgb0 rgb1 0 0, stif_upsample_image); by0..wx1: bilinear rows / columns / weights of the
 * image at every HR query row / column (as in stif_dec_tables). */
typedef struct {
  const float* img;
  int ih, iw;
  const int* by0; const int* by1; const float* wy0; const float* wy1;
  const int* bx0; const int* bx1; const float* wx0; const float* wx1;
} stif_dec_image;

/* Stage 1 (per HR pixel): feat_imnet -> HRfeat [n,HH,WW,64]; flow_imnet -> flow [n,HH,WW,4].
 * proj: [n,h,w,256] LR projections (P1 | P2 | P3 | P4) from stif_conv2d_nhwc (1x1, packed by
 * stif_pack_dec_proj).  mlp: packed by stif_pack_dec_mlp.  t: [n] query time per item. */
int stif_dec_stage1(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_image* img,
                    const float* t, float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, void* stream);

/* Stage 2 (per HR pixel): warp grids from flow, bilinear HRfeat / projections, encode_imnet
 * -> RGB, written NCHW [n,3,HH,WW] (LunaTokis output layout, unclamped). */
int stif_dec_stage2(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                    const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out_nchw,
                    int n, int h, int w, int HH, int WW, void* stream);
/* The same stages with flags = STIF_CONV_F16X3: every SIREN layer on split-fp16 MFMA (mlp packed by
 * stif_pack_dec_mlp_ex with the same flag); flags = 0 is stif_dec_stage1 / stif_dec_stage2.
 * status: optional device word (NULL = none), set to 1 by stage 2 in f16x3 mode when an RGB output or
 * the stage-1 flow it reads is not finite (an HRfeat / hidden activation outside the split range
 * propagates to the RGB; a flow_imnet one to the flow, which the warpgrid clamp would otherwise turn
 * into a finite grid). */
int stif_dec_stage1_ex(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_image* img,
                       const float* t, float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, int flags,
                       int* status, void* stream);
int stif_dec_stage2_ex(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                       const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out, int n, int h,
                       int w, int HH, int WW, int flags, int* status, void* stream);

/* out = sum_k pred_k * wgt_k (per HR pixel weights [HH*WW], shared by the n items): the
 * local ensemble's area blend (Sakuya_arch_test.py:1076-1084). pred_k / out: [n][3][HH][WW]. */
int stif_dec_blend4(const float* const* pred, const float* const* wgt, float* out, int n, int HH, int WW,
                    void* stream);

/* HRinp for decoding_test: F.upsample(x, scale_factor=s, mode='bilinear') (align_corners=False)
 * of the NCHW pair x [n][2][3][h][w] as NHWC [n][s*h][s*w][8] (rgb0 rgb1 0 0). */
int stif_upsample_image(const float* x_nchw, float* out, int n, int h, int w, int s, void* stream);

/* ---- video harness I/O (custom_video_test.py:88-103) ---- */

/* data.util.imresize_np(frame, scale, antialiasing) of nf cv2-style uint8 BGR HWC frames [nf][H][W][3]
 * (separable cubic, symmetric padding; data/util.py:302-371), written as the model input: RGB NCHW
 * float / 255 [nf][3][oH][oW].  wH [oH][PH], iH [oH] (first symmetric-padded row), sH (top padding)
 * and the W equivalents come from calculate_weights_indices (stif_amd.video.resize_tables). */
int stif_resize_frames(const unsigned char* bgr, float* out_rgb_nchw, int nf, int H, int W, int oH, int oW,
                       const float* wH, const int* iH, int PH, int sH, const float* wW, const int* iW, int PW, int sW,
                       void* stream);
/* (clamp(x, 0, 1) * 255).astype(uint8) of NCHW RGB frames [n][3][H][W] -> HWC uint8 [n][H][W][3]. */
int stif_frames_to_u8(const float* nchw, unsigned char* hwc, int n, int H, int W, void* stream);

/* ---- training batches (data/__init__.py:124-154 collate_function2, data/util.py:126-140 augment_a2) ---- */

/* n square crops of uint8 BGR HWC frames -> float RGB planes out [n][3][o][o]:
 *   imresize_np(crop, scale, True).astype(float32) / 255, then flip W, flip H, transpose H/W (in that order, as
 *   selected by flags), BGR -> RGB, HWC -> CHW.
 * Crop k is the G x G square whose top-left pixel is src + crop_off[k] (an element offset), its rows row_stride[k]
 * elements apart: a crop of a larger device-resident frame is read in place, a packed buffer of crops has
 * row_stride = 3 G.  crop_off and row_stride are device arrays.  w [o][P], idx [o] (first symmetric-padded index) and
 * s0 (leading padding) come from calculate_weights_indices for (G -> o) (stif_amd.video.resize_tables); H and W share
 * them.  The padding mirrors at the crop's edge and no byte outside a crop is read.  Before the augmentation the
 * values are bit-identical to stif_resize_frames of the crop (same fmaf order).  One launch, no workspace, no atomics.
 * STIF_E_INVALID before any launch: a null pointer; n, G, o or P < 1; s0 > G; unknown flag bits. */
enum { STIF_BATCH_HFLIP = 1, STIF_BATCH_VFLIP = 2, STIF_BATCH_ROT90 = 4 };
int stif_build_batch(const unsigned char* src, const long long* crop_off, const long long* row_stride, float* out,
                     int n, int G, int o, const float* w, const int* idx, int P, int s0, unsigned flags, void* stream);

/* ---- host-side weight packing (pure CPU, callable without a GPU) ---- */
enum { STIF_PACK_PLAIN = 0, STIF_PACK_OFFMASK = 1, STIF_PACK_LSTM = 2, STIF_PACK_WINO = 3, STIF_PACK_WINO_OFFMASK = 4,
       STIF_PACK_WINO_LSTM = 5, STIF_PACK_DCNSEP = 6, STIF_PACK_DCNPAIR = 7 };
/* OR'ed into a STIF_PACK_WINO* mode: the f16x3 split packing for stif_conv3x3_wino with
 * flags = STIF_CONV_F16X3 (same size in bytes) */
#define STIF_PACK_F16X3 16

/* Size in floats of a packed conv weight / bias for a packing mode. */
size_t stif_conv_weight_floats(int cout, int cin, int ks, int mode);
size_t stif_conv_bias_floats(int cout, int mode);
/* w_oihw: [cout][cin][ks][ks] (nn.Conv2d layout).  dst layout:
 * [slice][cin/8][ks*ks][nt][lane 64][4] -- the MFMA B fragments of one (slice, 8-channel chunk),
 * contiguous so the kernel copies them to LDS with LDS-DMA; a slice is 32*NT output channels
 * (NT = 7 for OFFMASK, 4 for LSTM, 2 otherwise), cout padded to a whole slice with zeros, and
 * output rows permuted per `mode` (OFFMASK: [group][tap][dy, dx, mask]; LSTM: gates i,f,o,g
 * of 32 hidden channels per slice).
 * STIF_PACK_WINO (3x3 only, for stif_conv3x3_wino): the Winograd-domain weights U = G g G^T
 * (F(2x2,3x3), computed in double) as [cout/64][cin/8][i 4][j 4][nt 2][lane 64][4], lane l of
 * (i, j, nt) holding U[i][j] of cout slice*64 + nt*32 + (l & 31), input channel
 * chunk*8 + 4(l >> 5) + e; cout padded to a multiple of 64.  STIF_PACK_WINO_OFFMASK: the same
 * with the OFFMASK row permutation (216 -> 256 rows).  STIF_PACK_WINO_LSTM: the same for the
 * ConvLSTMCell conv (128 -> 256) with packed cout 4h + gate = reference row gate*64 + h (gates
 * i, f, o, g; convlstm.py:49), so one 4-cout quad holds the four gates of hidden channel h.
 * STIF_PACK_WINO* | STIF_PACK_F16X3: U * 2^10 split into fp16 h = rne(U 2^10), l = rne(U 2^10 - h)
 * as [cout/64][cin/16][i 4][j 4][nt 2][plane h|l][lane 64][8 halves], lane l's element e holding
 * input channel 16 q + 8 (e >> 2) + 4 (l >> 5) + (e & 3) (the chunk pair of one f16 MFMA).
 * STIF_PACK_PLAIN | STIF_PACK_F16X3 (64 -> 64 3x3 only: the stif_dcn_nhwc core, and the 3x3
 * stride-2 convs of stif_conv2d_nhwc, with flags = STIF_CONV_F16X3): [group 8][tap pair 5][nt 2][plane h|l][lane 64][8 halves], element e
 * of lane l holding tap 2p + (l >> 5) (tap 9 = 0), input channel 8 group + e.
 * STIF_PACK_DCNSEP | STIF_PACK_F16X3 (conv_offset_mask 64 -> 216, 3x3, for stif_dcn_sep_nhwc): the MFMA
 * A operands [k 36][M-tile m 7][plane h|l][lane 64][8 halves] of W * 2^10, step k = 9 c + tap, lane l
 * holding row i = l & 31 of M-tile m and input channel 16 c + 8 (l >> 5) + e.  Row i is accumulator
 * register r = (i & 3) + 4 (i >> 3) of lane half h = (i >> 2) & 1; half h owns the deformable groups
 * h, h + 2, h + 4, h + 6 and its slot s = 16 m + r < 108 holds component s % 3 (dy, dx, mask) of tap
 * (s % 27) / 3 of group 2 (s / 27) + h (slots 108..111 zero).  Bias: [8][32] in the same row order.
 * STIF_PACK_DCNPAIR | STIF_PACK_F16X3 (the 64 -> 64 3x3 DCN weight of stif_dcn_sep_nhwc): [group pair
 * a 4][tap 9][nt 2][plane h|l][lane 64][8 halves], element e of lane l holding input channel
 * 8 (2 a + (l >> 5)) + e, cout nt * 32 + (l & 31). */
int stif_pack_conv_weight(const float* w_oihw, const float* b, int cout, int cin, int ks, int mode,
                          float* w_dst, float* b_dst);

/* The Winograd packer on the device, for weights that change every training step: all pointers are device
 * pointers, nothing is read back and nothing is copied through the host.  mode STIF_PACK_WINO or STIF_PACK_WINO |
 * STIF_PACK_F16X3, ks 3, cin = cout = 64 (anything else is STIF_E_INVALID); w_dst / b_dst sized by
 * stif_conv_weight_floats / stif_conv_bias_floats.  The bytes written are those stif_pack_conv_weight writes for
 * the same weight (the transform is evaluated in double in the same addition order, every product exact).
 * flags = STIF_PACK_DGRAD: packs the data gradient's weight w'[ci][co][kh][kw] = w[co][ci][2 - kh][2 - kw] with a
 * zero bias (b may be NULL then), so that stif_conv3x3_wino on grad_output computes grad_input.
 * status: device word, required with STIF_PACK_F16X3 (may be NULL otherwise): where the host packer returns
 * STIF_E_RANGE (a U = G g G^T outside |U| <= 65504 / 1024) the kernel ORs STIF_STATUS_PACK_RANGE into *status
 * (a vector atomic) and the packed bytes are unspecified -- pack and run that layer with STIF_PACK_WINO alone. */
#define STIF_PACK_DGRAD 1
#define STIF_STATUS_PACK_RANGE 16
int stif_pack_conv_weight_dev(const float* w_oihw, const float* b, int cout, int cin, int ks, int mode, int flags,
                              float* w_dst, float* b_dst, int* status, void* stream);
/* The fp32 STIF_PACK_PLAIN packing of a 64 -> 64 3x3 layer on the device (anything else is STIF_E_INVALID): byte
 * for byte what stif_pack_conv_weight(..., STIF_PACK_PLAIN) writes, sized by stif_conv_weight_floats /
 * stif_conv_bias_floats; b may be NULL (a zero bias).  With it the training forward of a stride-2 conv is
 * stif_conv2d_nhwc with no host packing and no synchronisation. */
int stif_pack_conv_plain_dev(const float* w_oihw, const float* b, int cout, int cin, int ks, float* w_dst,
                             float* b_dst, void* stream);
/* stif_pack_conv_weight_dev for one 64 x 64 block of a larger 3x3 weight: rows [co0, co0 + 64) and columns
 * [ci0, ci0 + 64) of the OIHW weight [cout][cin][3][3], cout 64 or 216 with cin 64 or 128, or the ConvLSTM cell's
 * [256][128] (eight blocks in row order are its pack, the four STIF_PACK_DGRAD row blocks of column block ci0 the
 * data gradient's 256 -> 64 weight of that input half), co0 / ci0 multiples of 64
 * inside it (anything else is STIF_E_INVALID before the launch); rows at or past cout read as zeros, and so does
 * their bias.  Writes one 64 -> 64 pack (stif_conv_weight_floats(64, 64, 3, mode) floats) at w_dst and 64 biases
 * (b[co0 ..], zeros with STIF_PACK_DGRAD) at b_dst; modes, flags and status as stif_pack_conv_weight_dev.  A Winograd
 * pack is [cout slice][cin chunk]..., so block packs laid end to end are the packs of wider layers: the two column
 * blocks of a [64][128] weight are its pack, the four row blocks of a [216][64] weight are its pack (216 rows padded
 * to 256), the four STIF_PACK_DGRAD row blocks of [216][64] are the data gradient's 256 -> 64 weight, and the
 * STIF_PACK_DGRAD pack of one column block of [64][128] is the data gradient's weight for that input half. */
int stif_pack_conv_block_dev(const float* w_oihw, const float* b, int cout, int cin, int co0, int ci0, int mode,
                             int flags, float* w_dst, float* b_dst, int* status, void* stream);
/* The packer of the 1x1 (64 | 64) -> 64 layers on the device: w_oihw [64][128][1][1], cout 64, cin 128, ks 1 (anything
 * else is STIF_E_INVALID).  mode STIF_PACK_PLAIN or STIF_PACK_PLAIN | STIF_PACK_F16X3 with ci0 = 0: byte for byte what
 * stif_pack_conv_weight(ks = 1) writes in that mode; where the host packer returns STIF_E_RANGE the kernel ORs
 * STIF_STATUS_PACK_RANGE into *status (required with STIF_PACK_F16X3).  flags = STIF_PACK_DGRAD (mode STIF_PACK_PLAIN,
 * ci0 = 0 or 64): the fp32 pack of the transposed 64 -> 64 layer w'[ci][co] = w[co][ci0 + ci] with a zero bias (b may
 * be NULL), so that the 1x1 conv of grad_output is the gradient of that input half. */
int stif_pack_conv1x1_dev(const float* w_oihw, const float* b, int cout, int cin, int ci0, int mode, int flags,
                          float* w_dst, float* b_dst, int* status, void* stream);

size_t stif_dec_proj_floats(void);   /* packed fp32 1x1 weight of the LR projection: [25][256][1][8]; the
                                        f16x3 packing: stif_conv_weight_floats(256, 200, 1, STIF_PACK_PLAIN | STIF_PACK_F16X3) */
int stif_pack_dec_proj(const float* feat_w0, const float* feat_b0, const float* flow_w0,
                       const float* enc_w0, float* w_dst, float* b_dst);
/* lr_image bit 0 clear: P2..P4 without the image columns (decoding_test samples a high-resolution
 * image); lr_image | STIF_DEC_REVOLUTIONS: the sine-layer factor is omega_0 / (2 pi) instead of omega_0
 * (pre-activations in revolutions), as the decoder stages run with STIF_CONV_F16X3 expect -- set it iff
 * the mlp was packed with STIF_CONV_F16X3 (the stages cannot check the pairing: a mismatch gives wrong first-layer
 * sines with no error, INTEGRATION.md "Decoder pairing rule"); lr_image | STIF_PACK_F16X3: the PLAIN | F16X3 1x1 packing for stif_conv2d_nhwc with
 * flags = STIF_CONV_F16X3 (split-fp16 k_conv1x1) */
#define STIF_DEC_REVOLUTIONS 2
int stif_pack_dec_proj_ex(const float* feat_w0, const float* feat_b0, const float* flow_w0,
                          const float* enc_w0, int lr_image, float* w_dst, float* b_dst);
size_t stif_dec_mlp_floats(void);
/* Packs every remaining feat/flow/encode_imnet weight (state-dict shapes, see stif_amd.weights)
 * in the order stif_dec_stage1/2 consume them. Pointers follow the Siren layer order:
 * feat: w0,b0,w1,b1,w2,b2,w3,b3; flow: same; enc: w0..w4, b0..b4 interleaved. */
int stif_pack_dec_mlp(const float* const* feat, const float* const* flow, const float* const* enc,
                      float* dst);
/* flags = STIF_CONV_F16X3: every 32x32 MFMA weight tile as a split-fp16 tile ([m 2][plane h|l][lane 64]
 * [8 halves] of W * 2^10, element e of half-tile m = feature F(8m + e, lane >> 5)) and the image tiles
 * scaled by 2^14, and the sine layers scaled by omega_0 / (2 pi) (revolutions: the stages evaluate
 * v_sin_f32(x - rint(x))), for stif_dec_stage1_ex / stif_dec_stage2_ex with the same flag; encode_imnet's
 * tiles are also stored a second time as 16x16x32 A operands for the 16-pixel stage 2 (dec_layout.h Q_*). */
int stif_pack_dec_mlp_ex(const float* const* feat, const float* const* flow, const float* const* enc,
                         float* dst, int flags);

const char* stif_last_error(void);
const char* stif_version(void);

/* ---- windowed decoding: any rectangle of the virtual HH x WW grid at the cost of that rectangle ---- */

/* A query rectangle of the virtual grid, the rectangle of the grid the HRfeat buffer holds, and where
 * stage 2 writes.  Zero-initialise, then fill: all-zero F fields mean F = the query rectangle, all-zero
 * out fields mean a dense [n][3][hh][ww] output. */
typedef struct {
  int y0, x0, hh, ww;      /* query rectangle: rows [y0, y0 + hh), columns [x0, x0 + ww); hh, ww >= 1 */
  int fy0, fx0, fh, fw;    /* F rectangle: hrfeat is [n][fh][fw][64], pixel (r, c) = grid pixel (fy0 + r, fx0 + c) */
  long long out_item;      /* stage-2 output addressing in elements: pixel (py, px) of the query rectangle, */
  long long out_plane;     /* channel c, item i is out[i * out_item + c * out_plane + py * out_pitch + px], */
  int out_pitch;           /* so a tile can be written straight into a larger [n][3][HH][WW] tensor */
} stif_dec_window;

/* stif_dec_stage1_ex over the query rectangle of `win`: HH, WW and the tables (stif_dec_image's too) stay those
 * of the whole virtual grid; pixel (py, px) of the rectangle uses the table entries y0 + py, x0 + px.  flow:
 * [n][hh][ww][4]; hrfeat: the pixel's row in the F layout (F must contain the query rectangle; with F = the
 * query rectangle that is [n][hh][ww][64]).  flow = NULL: feat_imnet only (HRfeat of the rectangle, e.g. of an
 * F rectangle larger than the window stage 2 is run for).  Tables with hr_y / hr_x are STIF_E_INVALID (the
 * windowed flow stage of a shifted query is stif_dec_flow_win). */
int stif_dec_stage1_win(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_image* img,
                        const float* t, float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, int flags,
                        int* status, void* stream, const stif_dec_window* win);
/* box[0..3] = ymin, ymax, xmin, xmax (inclusive) over all n items of every HRfeat corner (row, column) stage 2
 * reads for the query rectangle given its flow [n][hh][ww][4] -- the clamped corners of both warped grids,
 * zero-weight corners included.  F must contain this box. */
int stif_dec_bounds(const float* flow, const stif_dec_tables* tab, int* box, int n, int HH, int WW, void* stream,
                    const stif_dec_window* win);
/* stif_dec_stage2_ex over the query rectangle: flow [n][hh][ww][4], hrfeat in the F layout, RGB written through
 * out_item / out_plane / out_pitch.  Every HRfeat index is clamped into F before use; if one had to be, bit 1
 * (value 2) is OR'ed into *status (F was too small: the result is wrong, no read left the buffer).  Bit 0 as
 * stif_dec_stage2_ex. */
int stif_dec_stage2_win(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                        const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out, int n, int h,
                        int w, int HH, int WW, int flags, int* status, void* stream, const stif_dec_window* win);

/* ---- local ensemble over a window (decoding_localensemble, Sakuya_arch_test.py:962-1085): per shift k (k = 0..3
 * numbers the reference's shifts (-1,-1), (-1,1), (1,-1), (1,1)): stif_dec_stage1_win(flow = NULL) with the shifted
 * tables (hr_y = hr_x = NULL) over an F that holds the remap rectangle, stif_dec_flow_win, stif_dec_bounds, a
 * feat-only pass over a larger F if the box asks for one, stif_dec_stage2_blend_win -- the four shifts one after
 * the other on one stream (see stif_dec_stage2_blend_win for the order). ---- */

/* flow_imnet alone over the query rectangle, with the tables of a shifted query (hr_y / hr_x required): the HRfeat
 * operand of pixel (py, px) is the row of HR pixel (hr_y[py], hr_x[px]), read from hrfeat in the F layout.  F need
 * not contain the query rectangle; it must contain the remap rectangle [hr_y[y0], hr_y[y0 + hh - 1]] x
 * [hr_x[x0], hr_x[x0 + ww - 1]] (the tables are monotone).  Every index is clamped into F before use; if one had to
 * be, bit 2 (value 4) is OR'ed into *status (F was too small: the flow is wrong, no read left the buffer).
 * flow: [n][hh][ww][4], bit-identical to stif_dec_stage1_ex's flow with the same tables at the same pixels.
 * img must be NULL (STIF_E_INVALID otherwise). */
int stif_dec_flow_win(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_image* img,
                      const float* t, const float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, int flags,
                      int* status, void* stream, const stif_dec_window* win);

/* The blend of decode k into the output.  Zero-initialise, then fill.  rel_y[j] / rel_x[j]: the rel_y / rel_x
 * tables (stif_dec_tables, whole virtual grid) of shift j = 0..3 in the reference's order.  The weight of decode k
 * at (py, px) is computed in the epilogue, in fp32 with every operation rounded on its own:
 * a_j = |rel_y[j][py] * rel_x[j][px]| + 1e-9f, tot = ((a_0 + a_1) + a_2) + a_3, w_k = a_(3-k) / tot. */
typedef struct {
  int k;                       /* which of the four decodes this launch is: 0..3 */
  int accumulate;              /* 0: out = w_k * rgb (out is not read); 1: out = fma(rgb, w_k, out) */
  const float* rel_y[4];
  const float* rel_x[4];
} stif_dec_blend;

/* stif_dec_stage2_win with the local ensemble's blending epilogue: the first of a window's four launches
 * (accumulate = 0) stores w_k * rgb, the other three store fma(rgb, w_k, out), one after the other on one stream.
 * stif_dec_blend4 as built for gfx950 computes fma(p_3, w_3, fma(p_2, w_2, fma(p_0, w_0, p_1 * w_1))) (the
 * compiler contracts its first sum into the second product), so the launch order k = 1, 0, 2, 3 gives its bits;
 * the order 0, 1, 2, 3 gives the uncontracted sum's first rounding instead (a last-place difference).  Each
 * output element is written by one lane (no atomics).  img must be NULL.  Status bits as stif_dec_stage2_win. */
int stif_dec_stage2_blend_win(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                              const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out, int n,
                              int h, int w, int HH, int WW, int flags, int* status, void* stream,
                              const stif_dec_blend* blend, const stif_dec_window* win);

/* ---- time fields: every output pixel decoded at its own query time (LunaTokis.decoding with times[c] of shape
 * [bs, HH*WW], Sakuya_arch_test.py:364-459) ---- */

/* The query time of pixel (gy, gx) of the virtual HH x WW grid of item i is t[i * item + gy * row + gx * col]:
 * strides in elements, each >= 0, 0 broadcasts.  {t, 1, 0, 0} is the per-item vector the other entry points take;
 * {t, HH * WW, WW, 1} a dense [n][HH][WW] field; {t, 0, 1, 0} one time per row for every item.  A window does not
 * move the field: its pixel (py, px) reads the field at (y0 + py, x0 + px).  The values are not validated (the
 * reference imposes no range). */
typedef struct { const float* t; long long item, row, col; } stif_dec_time;

/* stif_dec_stage1_ex (win = NULL: the whole grid; flow must then be given or NULL as below) or stif_dec_stage1_win
 * (win given) with a time field: HRfeat of pixel q and its flow are computed with t(q).  flow = NULL: feat_imnet
 * only, e.g. over an F rectangle larger than the window -- the field is then read at F's pixels.  A pixel whose
 * field value is v gets bit for bit what the per-item call with t = v gives it.  STIF_E_INVALID, each with its
 * reason in stif_last_error: img != NULL, tables with hr_y / hr_x, a null t (the struct or its pointer), a negative
 * stride. */
int stif_dec_stage1_tf(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_image* img,
                       const stif_dec_time* t, float* hrfeat, float* flow, int n, int h, int w, int HH, int WW,
                       int flags, int* status, void* stream, const stif_dec_window* win);
/* stif_dec_stage2_ex (win = NULL) or stif_dec_stage2_win (win given) with a time field: pixel p gathers the HRfeat
 * rows at its warped grids -- each computed with its own pixel's time by stage 1 -- and adds w_t * t(p), as the
 * reference does when it grid-samples an HRfeat map built with a per-pixel time.  Status bits and the invalid
 * arguments as above. */
int stif_dec_stage2_tf(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                       const stif_dec_tables* tab, const stif_dec_image* img, const stif_dec_time* t, float* out, int n,
                       int h, int w, int HH, int WW, int flags, int* status, void* stream, const stif_dec_window* win);

/* ---- point queries: any set of pixels of the virtual grid, each at its own time, at the cost of those pixels.
 * The RGB of point (item i, row y, column x, time t) is bit for bit what stif_dec_stage1_ex / stif_dec_stage2_ex with
 * the per-item time t write at [i][:][y][x].  The eight HRfeat rows stage 2 gathers for a point (the corners of its
 * two warped grids) are computed with the point's own time -- unlike a time field, where a corner row carries the
 * corner pixel's time -- so every point is an independent sample of the scalar-time decode.  Corners are not shared
 * between points (two points at one pixel with different times have different corner rows): a point costs about
 * nine feat_imnet evaluations instead of one, and a dense block of pixels is cheaper as a window.
 * Per call: stif_dec_stage1_pts (flow, and the points' own HRfeat) -> stif_dec_corners_pts (the corner list)
 * -> stif_dec_stage1_pts over the corner list with flow = NULL (the compact HRfeat [n][npts][8][64])
 * -> stif_dec_stage2_pts.  Nothing is read back between them. ---- */

/* point p of item i: row y[i * y_item + p], column x[i * x_item + p], time t[i * t_item + p * t_point];
 * strides in elements, >= 0, 0 broadcasts; npts >= 1 points per item */
typedef struct { const int* y; const int* x; const float* t; long long y_item, x_item, t_item, t_point; int npts; } stif_dec_points;

/* Every kernel that reads y / x clamps them into the HH x WW grid before use; if it had to, bit 3 (value 8) is
 * OR'ed into *status (the value of that point is the clamped pixel's; no read left a buffer).  All three entry
 * points return STIF_E_INVALID, with the reason in stif_last_error, for a null pointer, npts < 1, n * 8 * npts
 * beyond INT_MAX, a negative stride and tables with hr_y / hr_x. */

/* Stage 1 over the points: hrfeat [n][npts][64] and flow [n][npts][4], each point's bit for bit those of
 * stif_dec_stage1_ex at its pixel with its time.  flow = NULL: feat_imnet only. */
int stif_dec_stage1_pts(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_points* pts,
                        float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, int flags, int* status,
                        void* stream);
/* The HRfeat corner pixels stage 2 gathers for every point given its flow [n][npts][4], as a point list of 8 * npts
 * entries per item: cy, cx (clamped rows / columns) and ct (the point's time) are [n][8 * npts]; entries 8 p + 0..3
 * are the corners (y0, x0), (y0, x1), (y1, x0), (y1, x1) of point p's first warped grid, 8 p + 4..7 those of its
 * second; corners of weight zero are listed too.  {cy, cx, ct, 8 * npts, 8 * npts, 8 * npts, 1, 8 * npts} is the
 * stif_dec_points of the feat-only pass. */
int stif_dec_corners_pts(const float* flow, const stif_dec_tables* tab, const stif_dec_points* pts, int* cy, int* cx,
                         float* ct, int n, int HH, int WW, int* status, void* stream);
/* Stage 2 over the points: hrfeat8 [n][npts][8][64] holds the corner rows in stif_dec_corners_pts' order, flow is
 * stage 1's; out [n][3][npts].  Bit 0 of *status as stif_dec_stage2_ex (OR'ed in, so bit 3 survives). */
int stif_dec_stage2_pts(const float* proj, const float* mlp, const float* hrfeat8, const float* flow,
                        const stif_dec_tables* tab, const stif_dec_points* pts, float* out, int n, int h, int w,
                        int HH, int WW, int flags, int* status, void* stream);

/* ---- local ensemble at points: point (item i, row y, column x, time t) is bit for bit what the four-shift
 * sequence above (stif_dec_stage2_blend_win over the whole grid with the per-item time t) leaves at [i][:][y][x].
 * Per shift k, in the launch order of stif_dec_stage2_blend_win, on one stream, with tab_k the tables of shift k and
 * plain_k the same without hr_y / hr_x: stif_dec_remap_pts (tab_k) -> stif_dec_stage1_pts (plain_k, the list
 * {ry, rx, t}, flow = NULL: the compact HRfeat operand [n][npts][64]) -> stif_dec_flow_pts (tab_k) ->
 * stif_dec_corners_pts (plain_k) -> stif_dec_stage1_pts over the corner list (plain_k, flow = NULL) ->
 * stif_dec_stage2_blend_pts (tab_k).  One shift's scratch is alive at a time; nothing is read back.
 * The three entry points return STIF_E_INVALID, with the reason in stif_last_error, for a null pointer, npts < 1,
 * n * 8 * npts beyond INT_MAX and a negative stride; y / x are clamped and flagged (bit 3) as above. ---- */

/* ry[i][p] = hr_y[y], rx[i][p] = hr_x[x] at point p's clamped row / column, both int32 [n][npts]: the HR pixel whose
 * HRfeat row the flow stage of the shifted query reads.  {ry, rx, t, npts, npts, t_item, t_point, npts} (t and its
 * strides the point list's) is the stif_dec_points of the feat-only pass that computes those rows.  Tables without
 * hr_y / hr_x are STIF_E_INVALID. */
int stif_dec_remap_pts(const stif_dec_tables* tab, const stif_dec_points* pts, int* ry, int* rx, int n, int HH, int WW,
                       int* status, void* stream);
/* flow_imnet alone over the points, with the tables of a shifted query (hr_y / hr_x required, as stif_dec_flow_win;
 * they are not read): the HRfeat operand of point p of item i is row [i][p] of hrfeat [n][npts][64].  flow:
 * [n][npts][4], each point's bit-identical to stif_dec_stage1_ex's flow with the same tables at its pixel and time. */
int stif_dec_flow_pts(const float* proj, const float* mlp, const stif_dec_tables* tab, const stif_dec_points* pts,
                      const float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, int flags, int* status,
                      void* stream);
/* stif_dec_stage2_pts with the local ensemble's blending epilogue (stif_dec_blend, the arithmetic and the launch
 * order of stif_dec_stage2_blend_win): the weight is taken at the point's clamped row / column of the virtual grid.
 * The tables of a shifted query are accepted (hr_y / hr_x are never read).  out [n][3][npts], each element written
 * by one lane (no atomics).  STIF_E_INVALID also for a bad blend: NULL, k outside 0..3, accumulate outside 0 / 1, a
 * null rel table.  Status bits as stif_dec_stage2_pts. */
int stif_dec_stage2_blend_pts(const float* proj, const float* mlp, const float* hrfeat8, const float* flow,
                              const stif_dec_tables* tab, const stif_dec_points* pts, float* out, int n, int h, int w,
                              int HH, int WW, int flags, int* status, void* stream, const stif_dec_blend* blend);

/* ---- evaluation: PSNR / SSIM of decoded frames against ground truth (myutils.py:1151-1174, util.py:105-174) ---- */

/* stif_metric_args.flags */
#define STIF_METRIC_Y 1      /* score the Y channel of bgr2ycbcr (data/util.py:181-202, not rounded); else the three
                                channels (PSNR over all of them at once, SSIM = mean of the per-channel SSIMs) */
#define STIF_METRIC_SSIM 2   /* also the SSIM sums (11 x 11 Gaussian, sigma 1.5, windows inside the image only) */
#define STIF_METRIC_FLOAT 4  /* myutils.calc_psnr (:269-271): squared error of the unquantised floats, data range 1,
                                against gt_f32; excludes _Y and _SSIM; gt_u8 is ignored */

/* Zero-initialise, then fill.  pred: the engine's output frames, fp32 RGB planes, unclamped; element (item i,
 * plane c, row y, column x) is pred[i * pred_item + c * pred_plane + y * pred_pitch + x], so the top-left crop of a
 * padded [n][3][HH][WW] output is scored in place.  pred_item = pred_plane = pred_pitch = 0 means a dense
 * [n][3][H][W].  gt_u8: cv2-style uint8 BGR HWC frames, byte (i, y, x, c) at gt_u8[i * gt_item + y * gt_pitch +
 * 3 * x + c]; gt_item = gt_pitch = 0 means dense [n][H][W][3].  gt_f32 (STIF_METRIC_FLOAT): fp32 RGB planes
 * addressed like pred through gtf_item / gtf_plane / gtf_pitch.
 * Quantised modes score q = rintf(clamp(pred, 0, 1) * 255.f) (utils.util.tensor2img: fp32, half to even)
 * against the ground truth's exact integers, in fp64. */
typedef struct {
  const float* pred;
  long long pred_item, pred_plane, pred_pitch;   /* elements */
  const unsigned char* gt_u8;
  long long gt_item, gt_pitch;                   /* bytes */
  const float* gt_f32;
  long long gtf_item, gtf_plane, gtf_pitch;      /* elements */
  int n, H, W;
  int flags;                                     /* STIF_METRIC_* */
} stif_metric_args;

/* Bytes of workspace stif_metric_psnr_ssim needs (four doubles per 32 x 32 tile of every scored plane); 0 for
 * sizes < 1 or an invalid flag combination.  Pure host. */
size_t stif_metric_workspace_size(int n, int H, int W, int flags);
/* out: device array [n][4] = { sum of squared errors, pixels summed (H W, or 3 H W in RGB / float mode), sum of
 * the SSIM map, windows summed ((H-10)(W-10) per plane; 0 without STIF_METRIC_SSIM or when H < 11 or W < 11) }
 * per item; PSNR = 20 log10(255 / sqrt(sse / npix)) (float mode: -10 log10(sse / npix + 1e-8)), SSIM =
 * ssim_sum / nwin (stif_amd.metrics.finish).  Two launches on `stream`, no host read-back (graph-capturable), no
 * floating-point atomics: repeated calls give identical bits.  Every argument is validated before the first
 * launch: STIF_E_INVALID for null pointers, sizes < 1, a pitch below the row length, overlapping planes or items,
 * bad flags; STIF_E_WORKSPACE for a missing or short workspace. */
int stif_metric_psnr_ssim(const stif_metric_args* args, double* out, void* workspace, size_t workspace_bytes,
                          void* stream);
/* The normalised 1-D window (cv2.getGaussianKernel(11, 1.5)) as the host computes it for the kernel. */
int stif_metric_window(double k[11]);

/* The float protocol, myutils.eval_metrics (:234-241): calc_psnr beside an SSIM of the frames clamped to [0, 1],
 * data range 1 (C1 = 1e-4, C2 = 9e-4), fp64 after the clamp, replicate padding of 5, so that every one of the
 * 3 H W positions is a centre.  STIF_FSSIM_VOLUME is myutils.ssim_matlab (:105-158): the RGB frame as a 3 x H x W
 * volume under an 11 x 11 x 11 window, padded on all three axes (over three channels the depth pass is a fixed
 * 3 x 3 channel mix).  STIF_FSSIM_PLANAR is myutils.ssim (:47-102): the 11 x 11 window per channel.  The window is
 * stif_metric_window's fp64 one; the reference builds its own in fp32 (gap: DESIGN.md section 3f). */
enum { STIF_FSSIM_VOLUME = 0, STIF_FSSIM_PLANAR = 1 };
/* Bytes of workspace stif_metric_float needs (four doubles per 32 x 32 tile of every channel); 0 for n < 1, H or
 * W < 11 (the reference's smaller window for smaller images is not reproduced) or an unknown mode.  Pure host. */
size_t stif_metric_float_workspace_size(int n, int H, int W, int mode);
/* args: pred / pred_* against gt_f32 / gtf_* (both fp32 RGB planes, unclamped), n, H, W; gt_u8 is ignored; flags
 * must be 0 or STIF_METRIC_FLOAT.  out: device array [n][4] = { sum of squared errors of the unclamped floats,
 * 3 H W, sum of the SSIM map, 3 H W } per item: PSNR = -10 log10(sse / npix + 1e-8), SSIM = ssim_sum / nwin
 * (stif_amd.metrics.finish with float_mode).  Two launches on `stream`, no host read-back (graph-capturable), no
 * floating-point atomics: repeated calls give identical bits.  Every argument is validated before the first
 * launch: STIF_E_INVALID for null pointers, n < 1, H or W < 11, an unknown mode, bad flags, a pitch below W,
 * overlapping planes or items, a misaligned out or workspace; STIF_E_WORKSPACE for a missing or short workspace. */
int stif_metric_float(const stif_metric_args* args, int mode, double* out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- video I/O: planar Y'CbCr (the frame payload of a YUV4MPEG2 stream) <-> the model's fp32 RGB planes ---- */

enum { STIF_YUV_BT601 = 0, STIF_YUV_BT709 = 1 };   /* stif_yuv_format.matrix: (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722) */

/* Zero-initialise, then fill.  Three planes per frame, luma width x height and chroma ceil(width / 2^sub_x) x
 * ceil(height / 2^sub_y); 4:4:4 = (0, 0), 4:2:2 = (1, 0), 4:2:0 = (1, 1).  depth 8: samples are bytes; 9..16:
 * little-endian uint16 (as Y4M stores them), planes / pitches / frame stride 2-byte aligned.  Sample values:
 * luma = yoff + yrange Y', chroma = 2^(depth-1) + crange C, with Y' = Kr R + Kg G + Kb B in [0, 1] and
 * Cb = (B - Y') / (2 (1 - Kb)), Cr = (R - Y') / (2 (1 - Kr)) in [-1/2, 1/2]; (yoff, yrange, crange) =
 * (16, 219, 224) * 2^(depth-8) with full_range = 0 and (0, 2^depth - 1, 2^depth - 1) with full_range = 1.  No
 * transfer function is applied: samples are display-referred, like the harness's 8-bit frames.
 * Both entry points take the three plane pointers of frame 0; frame i's planes start i * frame_stride bytes later.
 * pitch_y = pitch_c = 0 means dense rows, frame_stride = 0 means the dense Y4M frame, height * pitch_y +
 * 2 * chroma height * pitch_c bytes (Y | U | V).
 * Chroma siting: a chroma sample is taken to sit at the centre of its 2^sub_x x 2^sub_y box of luma pixels, in
 * every subsampled layout.  That is exact for Y4M's 420jpeg; for 420mpeg2 / 420 (horizontally co-sited) and
 * 420paldv (co-sited, Cb / Cr on alternate lines) it shifts the chroma by at most half a luma pixel. */
typedef struct {
  int width, height;           /* luma size, >= 1 (odd sizes give partial chroma boxes at the right / bottom edge) */
  int sub_x, sub_y;            /* log2 chroma subsampling, 0 or 1 */
  int depth;                   /* 8..16 bits per sample */
  int matrix;                  /* STIF_YUV_BT601 / STIF_YUV_BT709 */
  int full_range;              /* 0 limited ("TV"), 1 full ("PC") */
  long long pitch_y, pitch_c;  /* bytes between rows of the luma / chroma planes; 0 = dense */
  long long frame_stride;      /* bytes between frames; 0 = dense Y | U | V */
} stif_yuv_format;

/* n planar frames -> fp32 RGB planes in [0, 1]: element (i, c, y, x) is written at out[i * out_item +
 * c * out_plane + y * out_pitch + x] (the addressing of stif_metric_args.pred; all zero = a dense [n][3][H][W]), so
 * frames land directly in the top-left of a zero-filled, padded-to-4 [n][3][h_n][w_n] model input and nothing
 * outside the width x height rectangles is written.  Subsampled chroma is upsampled bilinearly (weights 3/4, 1/4
 * per subsampled axis, edge samples replicated; exact in fp32), then range expansion, matrix, clamp to [0, 1].
 * Validated before the launch: STIF_E_INVALID for a null pointer, n / width / height < 1, sub_x / sub_y / matrix /
 * full_range outside their values, depth outside 8..16, a pitch below the row length, a frame stride below a
 * plane's extent, misaligned 16-bit planes, overlapping out planes / items. */
int stif_yuv_to_rgb(const stif_yuv_format* fmt, const void* y, const void* u, const void* v, int n, float* out,
                    long long out_item, long long out_plane, long long out_pitch, void* stream);
/* n fp32 RGB frames (unclamped; element (i, c, y, x) at rgb[i * rgb_item + c * rgb_plane + y * rgb_pitch + x], all
 * zero = dense, so the top-left crop of a padded decoder output is converted in place) -> planar frames.  RGB is
 * clamped to [0, 1]; each chroma sample is the mean of Cb / Cr over the pixels of its box that exist, taken before
 * the quantisation; samples are rounded half to even (rintf, the rule of stif_metric_psnr_ssim's tensor2img) and
 * clamped to [0, 2^depth - 1].  Arithmetic is fp32 up to 10 bits and fp64 above (fp32's rounding error reaches
 * 4e-3 of a sample step at 16 bits).  Validation as stif_yuv_to_rgb. */
int stif_rgb_to_yuv(const stif_yuv_format* fmt, const float* rgb, long long rgb_item, long long rgb_plane,
                    long long rgb_pitch, int n, void* y, void* u, void* v, void* stream);

/* ---- scene cuts: how much the picture changes between adjacent frames of a clip ---- */

/* Bytes of workspace stif_scene_sad needs (one 64-bit partial sum per pair and workgroup; a function of the shape
 * alone); 0 for n < 2 or H, W < 1.  Pure host. */
size_t stif_scene_workspace_size(int n, int H, int W);
/* rgb: n >= 2 frames of fp32 RGB planes, element (i, c, y, x) at rgb[i * item + c * plane + y * pitch + x] (the
 * addressing of stif_metric_args.pred; all zero = a dense [n][3][H][W]), so the H x W rectangle in the top-left of
 * a padded [n][3][h_n][w_n] model input is scored in place; nothing outside the rectangle is read.
 * sad: device array [n - 1]; sad[i] = the sum over the rectangle of |q_i - q_i+1|, q the 8-bit luma of a pixel, in
 * fp32 without FMA contraction: r, g, b = fminf(fmaxf(v, 0), 1) (a NaN becomes 0); y = (0.299f r + 0.587f g) +
 * 0.114f b; q = min((int)rintf(y * 255.f), 255).  From q on the arithmetic is integer and the totals 64-bit (an 8K
 * pair going black to white sums to 8,460,288,000), so the result is exact, the same for every summation order and
 * every call, and equal to a host restatement to the last bit.  sad / (255 H W) is the mean luma change in [0, 1].
 * Two launches on `stream`, no atomics, no host read-back, no allocation (graph-capturable); each frame is read
 * once per 8 pairs.  Every argument is validated before the first launch: STIF_E_INVALID for null pointers, n < 2,
 * H or W < 1 (or H W > 2^48), a pitch below W, overlapping planes or items, a sad or workspace that is not 8-byte
 * aligned; STIF_E_WORKSPACE for a missing or short workspace. */
int stif_scene_sad(const float* rgb, long long item, long long plane, long long pitch, int n, int H, int W,
                   unsigned long long* sad, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STIF_H */
