/*
 * include/ossid_hip.h -- C ABI of libossid_hip.so, the MI355X (gfx950) drop-in for OSSID's hot path.
 *
 * The reference (r-pad/OSSID_code) is pure Python and has no FFI of its own: each
 * entry point below names the Python interface it stands behind (paths relative to
 * /root/reference/python/ossid). INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory,
 *     including workspaces (sizes from the *_workspace_bytes queries); nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work;
 *   - return 0 on success, a negative errno-style code otherwise (OSSID_EINVAL bad argument,
 *     OSSID_ELAUNCH a HIP launch error); no exceptions cross the boundary;
 *   - thread-safe for distinct streams; no global mutable state;
 *   - Zephyr entry points (ossid_zephyr_*, ossid_pn2_*): all arithmetic is IEEE binary32 with the operation order
 *     fixed by SPEC.md, so results are bit-identical to oracle/zephyr_oracle.c. DTOID entry points: binary32 tensors
 *     and accumulation; the convolution kernels' products as documented at ossid_conv_desc (`exact`).
 */
#ifndef OSSID_HIP_H
#define OSSID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSSID_OK 0
#define OSSID_EINVAL (-22)
#define OSSID_ELAUNCH (-5)

/* The version of the struct layouts and signatures below; bumped whenever one changes (3: ossid_conv_desc gained
 * scratch / scratch_bytes / exact; 5: ossid_wgrad_desc gained dy_add / dy_add_scale / dy_add_shift, ossid_dense_dgrad1_acc its dz_add arguments; 6: ossid_seq_replay / ossid_seq_op, ossid_bn_fold_bwd's zero_row). A binding compares it with ossid_abi_version() when it loads the library. */
#define OSSID_ABI_VERSION 6

/* library / device probe: returns OSSID_ABI_VERSION of the build; arch_out_host (may be NULL, >=32 bytes)
 * receives the gcnArchName of the current device, e.g. "gfx950:sramecc+:xnack-". */
int ossid_abi_version(char* arch_out_host, int len);

/* ---------------------------------------------------------------------------------------------
 * Z0  networkInference preprocessing          utils/zephyr_utils.py:13-14
 * cv2.GaussianBlur(img,(5,5),0) on u8 RGB [H,W,3] (blur=1) then /255 -> float, interleaved with
 * depth [H,W] (metres, 0 = invalid) into the staged frame rgbd[H,W,4] = (r,g,b,depth).
 * --------------------------------------------------------------------------------------------- */
int ossid_zephyr_prep_frame_u8(const uint8_t* img_rgb, const float* depth, int H, int W, int blur,
                               float* rgbd, void* stream);
/* same, for callers that already hold the float image (the tensor getPointNetData receives,
 * utils/zephyr_utils.py:14): img_rgb is float [H,W,3] in [0,1]. */
int ossid_zephyr_prep_frame_f32(const float* img_rgb, const float* depth, int H, int W, float* rgbd,
                                void* stream);

/* model table: tab[M][12] = (point xyz, normal xyz, HSV of the model colour, 3 pad)
 * from model_points / model_normals / model_colors [M,3] (utils/zephyr_utils.py:18-20). */
int ossid_zephyr_prep_model(const float* points, const float* normals, const float* colors_rgb, int M,
                            float* tab, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Z1  zephyr.utils.projectPointsUv(pose_hypos, model_points, meta_data)
 *     call site utils/zephyr_utils.py:58; K2meta utils/__init__.py:148-156
 * transforms [N,4,4] row-major float, points [M,3] -> uv [N,M,2] int32, uv[...,0]=x(col),
 * uv[...,1]=y(row); (-1,-1) marks a point at or behind the camera plane.
 * --------------------------------------------------------------------------------------------- */
int ossid_zephyr_project_uv(const float* transforms, const float* points, int N, int M, float fx, float fy,
                            float cx, float cy, int32_t* uv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Z2  ScoreDataset.getPointNetData(data, return_uv_original)   call site utils/zephyr_utils.py:31
 * (a) free-space-violation count per hypothesis, the input of the inconst_ratio_th filter
 *     (scripts/online_learning.py:174,184,196; utils/zephyr_utils.py:42-43);
 * (b) features of the hypotheses sel[0..Nsel) (sel NULL = identity):
 *     point_x[Nsel][M][8] = (x, y, 0, dH, dS, dV, dD, cosN), uv_original[Nsel][M][2] (may be NULL).
 * interp: 0 nearest pixel (default), 1 bilinear colour/depth.
 * --------------------------------------------------------------------------------------------- */
int ossid_zephyr_inconst_count(const float* rgbd, int H, int W, const float* transforms, int N,
                               const float* tab, int M, float fx, float fy, float cx, float cy,
                               float margin, int32_t* count, void* stream);
int ossid_zephyr_featurize(const float* rgbd, int H, int W, const float* transforms, const int32_t* sel,
                           int Nsel, const float* tab, int M, float fx, float fy, float cx, float cy,
                           int interp, float* point_x, int32_t* uv_original, void* stream);

/* SURVEY 8f-2 (the step right before Z0): per-hypothesis ADD / ADI pose error
 *   pp_err = [err_func(R, t, R_gt, t_gt, model_points) for mat in poses_all]       scripts/online_learning.py:452
 * err_func = zephyr.utils.metrics.add (symmetric=0) or adi (symmetric=1); float64 like the numpy reference.
 * transforms [N,4,4], transform_gt [4,4], points [M,3] (M*24 B <= 150 KB for ADI) -> err [N]. */
int ossid_pose_errors(const double* transforms, const double* transform_gt, const double* points, int N, int M,
                      int symmetric, double* err, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Z3  zephyr.models.pointnet2.PointNet2SSG.forward({"point_x": ...})
 *     ctor scripts/online_learning.py:212-227; call utils/zephyr_utils.py:34
 * Stage entry points (pointnet2_ops: furthest_point_sample, ball_query) and the whole scorer.
 * --------------------------------------------------------------------------------------------- */
/* xyz [B][n][stride] (first 3 floats of each row) -> idx [B][npoint], new_xyz [B][npoint][3] */
int ossid_pn2_fps(const float* xyz, int stride, int B, int n, int npoint, int32_t* idx, float* new_xyz,
                  void* stream);
/* idx [B][npoint][nsample], nsample must be 64 */
int ossid_pn2_ball_query(const float* xyz, int stride, int B, int n, const float* new_xyz, int npoint,
                         float radius, int nsample, int32_t* idx, void* stream);

/* Packed weight blob (built on the host by ossid_code_amd.zephyr.pack_pn2_weights, uploaded once):
 * float offsets into `blob` of the 12 layers' packed weights and biases, SPEC.md 4.3/4.4. */
typedef struct ossid_pn2_weights {
    const float* blob;
    int64_t w_off[12];
    int64_t b_off[12];
    int64_t wxyz2_off; /* SA2 L1 xyz columns, [3][128] */
    int32_t npoint1, npoint2; /* 512, 128 (npoint2 % 32 == 0, npoint1 % 32 == 0) */
    float radius1, radius2;   /* 0.2, 0.4 */
} ossid_pn2_weights;

size_t ossid_pn2_workspace_bytes(int B, int M, int npoint1, int npoint2);

/* point_x [B][M][8] -> scores [B]. workspace >= ossid_pn2_workspace_bytes(...), 256-byte aligned.
 * dbg_* (all may be NULL) receive copies of stage results for parity tests:
 * fps1 [B][np1] i32, ball1 [B][np1][64] i32, feat1 [B][np1][128], fps2 [B][np2] i32,
 * ball2 [B][np2][64] i32, feat2 [B][np2][256], feat3 [B][1024]. */
int ossid_pn2_score(const float* point_x, int B, int M, const ossid_pn2_weights* w, void* workspace,
                    size_t workspace_bytes, float* scores, int32_t* dbg_fps1, int32_t* dbg_ball1,
                    float* dbg_feat1, int32_t* dbg_fps2, int32_t* dbg_ball2, float* dbg_feat2,
                    float* dbg_feat3, void* const* stage_events_host, void* stream);

/* Workgroups in the grid of the two persistent kernels (sa1_kernel, sa2_kernel) of every later ossid_pn2_score call
 * of the process. 0, the default and what every product path uses: one workgroup per compute unit. A test sets a few
 * workgroups to give every wave a long slice of centres at a small batch; the results do not depend on it.
 * OSSID_EINVAL: workgroups outside [0, 65536] (nothing changed). */
int ossid_pn2_set_persistent_grid(int workgroups);

/* Kernel order of ossid_pn2_score; with stage_events_host != NULL (an array of OSSID_PN2_NSTAGES+1 hipEvent_t made
 * by ossid_event_create) event[i] is recorded on `stream` before stage i and event[NSTAGES] after the last, so a
 * caller can time each kernel of the launch it is actually measuring (bench.py's roofline leg). */
#define OSSID_PN2_NSTAGES 9
/* "fps1,ball1,sa1,p2,fps2,ball2,sa2,sa3,fc" */
const char* ossid_pn2_stage_names(void);

int ossid_event_create(void** event_out_host);
int ossid_event_destroy(void* event);
int ossid_event_record(void* event, void* stream);
/* waits for `stop`, then *ms_out_host = elapsed(start, stop) */
int ossid_event_elapsed_ms(void* start, void* stop, float* ms_out_host);

/* Names of the kernels the scorer launches, for profile post-processing (static string). */
const char* ossid_pn2_kernel_names(void);

/* ---------------------------------------------------------------------------------------------
 * Z3t  PointNet2SSG in training mode (csrc/pn2_train.hip, SPEC.md 12)
 *     the module scripts/online_learning.py:212-227 builds and loads; restates pointnet2_ops' PointnetSAModule,
 *     SharedMLP (Conv2d 1x1 no bias, BatchNorm2d, ReLU) and the classification head with batch-statistics BatchNorm
 *     and dropout, in TORCH's channel order (xyz first), and the backward pass to every parameter. zephyr's own
 *     training recipe is in neither tree: unpinned.
 * Layers 0..10 are the BatchNorm layers (SA1 x3, SA2 x3, SA3 x3, FC x2), layer 11 the last linear layer.
 * w[l] is torch's [cout][cin] matrix. run_mean / run_var (each may be NULL) are updated in place as torch does
 * (momentum 0.1, unbiased variance): hand in staging copies and copy_ them into the module's buffers.
 * --------------------------------------------------------------------------------------------- */
typedef struct ossid_pn2_train_params {
    const float* w[12];
    const float* gamma[11];
    const float* beta[11];
    const float* bias;
    float* run_mean[11];
    float* run_var[11];
    int32_t npoint1, npoint2;
    float radius1, radius2;
} ossid_pn2_train_params;

typedef struct ossid_pn2_train_grads {
    float* w[12];
    float* gamma[11];
    float* beta[11];
    float* bias;
} ossid_pn2_train_grads;

/* The decisions the forward took (every pointer may be NULL): relu[l] u8 [rows of layer l][C_l], 1 where the ReLU
 * passed; argmax[m] i32 [B][npoint][C] of the three poolings (the row within the group: sample 0..63 for SA1 and
 * SA2, point 0..npoint2-1 for SA3); the sampling and grouping indices as ossid_pn2_score exports them. */
typedef struct ossid_pn2_train_dbg {
    uint8_t* relu[11];
    int32_t* argmax[3];
    int32_t* fps1;
    int32_t* ball1;
    int32_t* fps2;
    int32_t* ball2;
} ossid_pn2_train_dbg;

/* 0 for a shape the training path refuses (B < 2, M < npoint1, npoint % 32 != 0, npoint1 < npoint2). */
size_t ossid_pn2_train_workspace_bytes(int B, int M, int npoint1, int npoint2);

/* point_x [B][M][8], keep_mask u8 [B][256] (1 = kept; kept values are scaled by 1/(1-p_drop)) -> scores [B].
 * The workspace (>= ossid_pn2_train_workspace_bytes, 256-byte aligned) keeps what the backward pass needs.
 * OSSID_EINVAL: a refused shape, a short or misaligned workspace, a NULL parameter. */
int ossid_pn2_train_forward(const float* point_x, int B, int M, const ossid_pn2_train_params* w,
                            const uint8_t* keep_mask, float p_drop, void* workspace, size_t workspace_bytes,
                            float* scores, const ossid_pn2_train_dbg* dbg, void* stream);
/* dscores [B] -> the gradient of every parameter (fresh values, not accumulated), from the workspace the forward
 * call left. It works in place on the workspace: ONE backward per forward. */
int ossid_pn2_train_backward(const float* dscores, int B, int M, const ossid_pn2_train_params* w, float p_drop,
                             void* workspace, size_t workspace_bytes, const ossid_pn2_train_grads* g, void* stream);

/* The stage kernels on their own (row-major f32 matrices):
 * Z[R][C] = X[R][Kp] (columns 0..Kr) . W[C][Kr]^T;  dX[R][N] = dZ[R][C] . W[C][ldw] (columns 0..N);
 * dW[C][Kr] = dZ[R][C]^T . X[R][Kp] (columns 0..Kr), split over rows and combined in split order. */
int ossid_pn2_train_linear_fwd(const float* X, int R, int Kp, const float* W, int Kr, int C, float* Z, void* stream);
int ossid_pn2_train_linear_dgrad(const float* dZ, int R, int C, const float* W, int ldw, int N, float* dX,
                                 void* stream);
size_t ossid_pn2_train_wgrad_workspace_bytes(int R, int C, int Kr);
int ossid_pn2_train_linear_wgrad(const float* dZ, int R, int C, const float* X, int Kp, int Kr, float* dW,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* out[b][i][:] = sum over e (ascending) with idx[b][e] == i of dG[b][e][:]; dG [B][E][Cf], idx [B][E], out [B][n][Cf] */
int ossid_pn2_train_ungroup(const float* dG, const int32_t* idx, int B, int E, int n, int Cf, float* out,
                            void* stream);
/* per-channel batch mean, 1/sqrt(biased variance + 1e-5) and (var may be NULL) the biased variance of Z[R][C], C <= 1024 */
size_t ossid_pn2_train_bn_stats_workspace_bytes(void);
int ossid_pn2_train_bn_stats(const float* Z, int R, int C, void* workspace, size_t workspace_bytes, float* mean,
                             float* rstd, float* var, void* stream);
/* out[g][c] = max over s < S of relu(bn(Z[g*S+s][c])), argmax = the first such s */
int ossid_pn2_train_bn_relu_pool(const float* Z, int G, int S, int C, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, float* out, int32_t* argmax, void* stream);

/* =============================================================================================
 * DTOID ops (paths under /root/reference/python/ossid/models/dtoid)
 * ============================================================================================= */

/* D5  conv2d_dw_group(x, kernel, padding=1)      network.py:186-192 (backbone) and :365-371 (head)
 * F.conv2d(x.view(1,B*C,H,W), k.view(B*C,1,3,3), groups=B*C, padding=1): per-plane 3x3 cross-correlation with a
 * data-dependent kernel. planes = B*C; x, out, dout, dx [planes][H][W]; k, dk [planes][3][3].
 * _bwd_x: gradient w.r.t. x; _bwd_k: gradient w.r.t. the kernel (gradients flow to both operands). */
int ossid_dw_xcorr_fwd(const float* x, int x_planes, const float* k, int planes, int H, int W, float* out,
                       void* stream);   /* x_planes = planes, or C when ONE image [C][H][W] is shared by all B kernels */
/* the same correlation, channels-last, ONE image x [H][W][channels] against `batch` kernel sets k [batch][channels][3][3]
 * (test time: the image broadcast over the templates) -> out [batch][H][W][channels]; channels % 4 == 0 */
int ossid_dw_xcorr_nhwc_bcast(const float* x, const float* k, int batch, int channels, int H, int W, float* out,
                              void* stream);
int ossid_dw_xcorr_bwd_x(const float* dout, const float* k, int planes, int H, int W, float* dx, void* stream);
int ossid_dw_xcorr_bwd_k(const float* x, const float* dout, int planes, int H, int W, float* dk, void* stream);

/* D4, D6-D8  the dense convolutions at test time: the head's 3x3 layers (network.py:102-110, :135-143, :288-326)
 * and the DenseNet-121 blocks of the image backbone (network.py:164-184), channels-last, f32 in and out, on the matrix cores
 * (arithmetic of the reduction: `exact`, below).
 *   out[b][y][x][out_channel_offset + co] = post( act( bias[co] + sum_{ci,tap} w[co][ci][tap] * pre(x)[b][y+dy][x+dx][ci] ) )
 * taps 9: 3x3 / stride 1 / padding 1 (zero halo);  taps 1: 1x1.
 * pre  = x * pre_scale[ci] + pre_shift[ci] (then ReLU if pre_relu) on real pixels only -- eval-mode BatchNorm(+ReLU)
 *        in FRONT of the conv (DenseNet's BN-ReLU-Conv); NULL = identity.
 * act  = 0 none, 1 ELU(alpha 1), 2 ReLU (SqueezeNet's Fire modules);  post = * post_scale[co] + post_shift[co] -- eval-mode BatchNorm BEHIND the ELU
 *        (`norm(F.elu(conv(x)))`); NULL = identity.
 * src_height/width > 0 (3x3 only): x is [B][src_h][src_w][..] and is nearest-neighbour up-sampled to [H][W] on the fly
 *        (F.interpolate(mode="nearest") in front of the conv, network.py:354-357).
 * in_channel_stride / out_channel_stride (0 = cin / cout) and out_channel_offset let a layer read the first cin channels of
 *        a wider resident buffer and append its output to it in place (DenseNet concatenation without torch.cat).
 * taps 4: the four PHASES of a 3x3 / pad 1 convolution applied to a 2x nearest-neighbour up-sampled input (the decoder,
 *        network.py:354-356): output pixel (2i+a, 2j+b) only sees source pixels (i+a-1, i+a) x (j+b-1, j+b), so each phase
 *        is a 2x2 convolution of the SOURCE with row/column-merged weights -- 4/9 of the multiply-adds. height/width are
 *        the SOURCE size, out is [B][2*height][2*width][..]; wpk = four ossid_conv_pack_weights(.., taps 4) sets, phase
 *        2a+b, of the merged [cout][cin][2][2] kernels (rows: a=0 -> (w0, w1+w2), a=1 -> (w0+w1, w2); columns likewise).
 * cin % 16 == 0; cout, strides and offset % 4 == 0. wpk = ossid_conv_pack_weights(w [cout][cin][kh][kw]). */
typedef struct ossid_conv_desc {
    const float* x;
    const float* wpk;
    const float* bias;
    const float* pre_scale;
    const float* pre_shift;
    const float* post_scale;
    const float* post_shift;
    float* out;
    int32_t batch, height, width, cin, cout, taps, act, pre_relu;
    int32_t src_height, src_width, in_channel_stride, out_channel_stride, out_channel_offset;
    int32_t pre_batch_stride;   /* floats between the pre_scale / pre_shift rows of consecutive images; 0 = one row */
    int64_t in_batch_stride;    /* floats between consecutive images of x; < 0 = dense (src_h * src_w * channel stride);
                                   0 = ONE image shared by the whole batch (a per-image pre-affine then makes each
                                   batch entry a different affine view of it: image_feat * avg_t, image_feat - avg_t
                                   of network.py:344-347 without materialising them) */
    /* Scratch a launch may use (optional): the Winograd entry's tail split (ossid_conv3x3_wino_workspace_bytes) keeps the
     * raw sums of its slices here; -DOSSID_TIMING diagnostic builds write per-wave time stamps. scratch_bytes = its size. */
    void* scratch;
    int64_t scratch_bytes;
    /* Arithmetic of the reduction in ossid_conv_nhwc_fwd (csrc/conv.hip). 0 (default): every f32 product w*x is formed as
     * three bf16 matrix-core products (w = hi + lo, x = hi + lo as bf16 pairs; w_lo*x_hi + w_hi*x_lo + w_hi*x_hi accumulated
     * in f32; the dropped lo*lo term is ~2^-16 of a product): ~5e-6 of the output scale against float64, tests hold 2e-5.
     * 1: v_mfma_f32_32x32x2_f32, exact f32 products (~1e-6), 5x the matrix-pipe time. 2: the three-way split -- operands as
     * three bf16 pieces (24 significant bits: the f32 value itself), six products, f32-level accuracy (~1e-6) at 2x the
     * pipe time of form 0 -- for layers whose output feeds a hard decision that a later pass repeats (the training forward
     * of the ReLU / max-pool networks: a pre-activation that lands on the other side of zero changes which units the
     * gradient flows through). wpk must be packed for the same form (ossid_conv_pack_weights_form; form 2 needs
     * ossid_conv_packed_floats_form floats, 1.5x the others). A library built with -DOSSID_CONV_F32 runs every launch exact;
     * ossid_conv_split_bf16() says whether the split form exists. The Winograd entry ignores the field (its own build
     * switch, below). */
    int32_t exact;
} ossid_conv_desc;
int ossid_conv_split_bf16(void);
size_t ossid_conv_packed_floats(int Cout, int Cin, int taps);
size_t ossid_conv_packed_floats_form(int Cout, int Cin, int taps, int exact);
/* w [Cout][Cin][taps] -> the operand layout of ossid_conv_nhwc_fwd (csrc/pack.hip). dgrad != 0: the layer
 * of the DATA gradient (Cin output channels, Cout reduction channels, taps reversed; needs ossid_conv_packed_floats(Cin,
 * Cout, taps) floats). exact: the form of the launches that will read it. ossid_conv_pack_weights = (dgrad 0, exact 0). */
int ossid_conv_pack_weights_form(const float* w, int Cout, int Cin, int taps, int dgrad, int exact, float* wpk, void* stream);
int ossid_conv_pack_weights(const float* w, int Cout, int Cin, int taps, float* wpk, void* stream);
int ossid_conv_nhwc_fwd(const ossid_conv_desc* desc_host, void* stream);

/* D6-D8 / D16  the same 3x3 convolution (stride 1, pad 1; ossid_conv_desc with taps = 9, no fused up-sampling, no
 * training extras) as Winograd F(2x2, 3x3): 16 multiplies per 2x2 output tile and channel pair instead of 36, f32
 * throughout (csrc/wino.hip; results differ from ossid_conv_nhwc_fwd by rounding only). Stands behind the same nn.Conv2d
 * layers (network.py:102-110, :135-143, :288-326) and their data gradients in the finetune step. desc->wpk must be the
 * layout of ossid_conv_pack_weights_wino: U = G g G^T of w [Cout][Cin][3][3]; dgrad != 0 packs the data gradient's layer
 * (Cin output channels, Cout reduction channels, filter rotated by 180 degrees; the desc then carries cin = Cout,
 * cout = Cin). The reduction channel count must be a multiple of 16.
 * Arithmetic of the channel reduction: by default every f32 product U*V is formed as three bf16 matrix-core products
 * (U = hi + lo, V = vh + vl as bf16 pairs; lo*vh + hi*vl + hi*vh accumulated in f32; the dropped lo*vl term is ~2^-16 of
 * a product): measured 7e-6 of the output scale against float64, tests hold <= 2e-5. A library built with
 * -DOSSID_WINO_F32 runs the same layout on v_mfma_f32_32x32x2_f32 (1e-6). ossid_conv_wino_split_bf16 says which. */
int ossid_conv_wino_split_bf16(void);
size_t ossid_conv_wino_packed_floats(int Cout, int Cin);
int ossid_conv_pack_weights_wino(const float* w, int Cout, int Cin, int dgrad, float* wpk, void* stream);
int ossid_conv3x3_wino_fwd(const ossid_conv_desc* desc_host, void* stream);
/* Scratch the Winograd launch wants for cutting the TAIL of its grid along the reduction (csrc/wino.hip: the last, partial
 * round of resident workgroups runs as ks slices per workgroup + a finishing launch; 1 576 workgroups on 512 slots cost
 * ~3.3 rounds instead of 4). 0 = no split planned for this shape. Pass the buffer in desc->scratch and its size in
 * desc->scratch_bytes (for the pair entry: in the first descriptor); without it the launch runs whole
 * workgroups. Results are bit-reproducible either way (fixed summation order), but differ in rounding between the two forms. */
size_t ossid_conv3x3_wino_workspace_bytes(const ossid_conv_desc* desc);
size_t ossid_conv3x3_wino_pair_workspace_bytes(const ossid_conv_desc* d0, const ossid_conv_desc* d1);
/* two independent layers (the i-th convolutions of the classification and the regression trunk, network.py:113-121 /
 * :146-154) in ONE grid: their workgroups fill the chip's slots together instead of each launch ending in a ragged round */
int ossid_conv3x3_wino_fwd_pair(const ossid_conv_desc* desc0_host, const ossid_conv_desc* desc1_host, void* stream);

/* D6 (tail)  the last two layers of the segmentation decoder in one launch (network.py:357-362):
 *   out[b][y][x] = b2 + conv3x3_{16->1}( post( ELU( b1 + conv3x3_{32->16}( nearest_upsample(x -> [H][W]) ) ) ) )
 * x [B][src_height][src_width][in_channel_stride] channels-last (the first 32 channels are read); w1p =
 * ossid_seg_tail_pack_weights(w1 [16][32][3][3]); post = * post_scale[16] + post_shift[16] (eval-mode BatchNorm);
 * w2 [16][3][3] (the [1][16][3][3] weight); b2 [1] (device, may be NULL); out [B][H][W]. Both convolutions zero-pad at the [H][W] border. The
 * 16-channel full-resolution tensor is never materialised. Returns OSSID_EINVAL when the up-sampling ratio is
 * below ~1.5 (the source footprint of a tile would not fit the staged patch): run the two layers separately then.
 * Arithmetic: the 32 -> 16 convolution on split-bf16 matrix-core products (as ossid_conv_desc.exact = 0: 8e-6 of the output
 * scale measured against float64; -DOSSID_SEGTAIL_F32 builds: exact f32, 1e-6), the 16 -> 1 convolution as f32 fmaf chains. */
int ossid_seg_tail_split_bf16(void);
size_t ossid_seg_tail_packed_floats(void);
int ossid_seg_tail_pack_weights(const float* w1, float* w1p, void* stream);
int ossid_seg_tail_fwd(const float* x, int batch, int src_height, int src_width, int in_channel_stride, int height,
                       int width, const float* w1p, const float* b1, const float* post_scale, const float* post_shift,
                       const float* w2, const float* b2, float* out, void* stream);

/* D16  weight gradient of the 3x3 / stride 1 / pad 1 convolution (loss.backward() of the finetune step,
 * scripts/online_learning.py:670-672): dw[co][ci][ky][kx] (+)= sum_{b,y,x} dy[b][y][x][co] * x[b][y+ky-1][x+kx-1][ci].
 * x [B][H][W][in_channel_stride], dy [B][H][W][dy_channel_stride] channels-last (0 = Cin / Cout); dw in torch layout
 * [Cout][Cin][3][3]; accumulate != 0 adds to dw. Split-K partial slabs in `workspace`, summed in a fixed order
 * (bit-reproducible). The data gradient needs no entry point of its own: it is ossid_conv_nhwc_fwd on dy with the
 * 180-degree-rotated, transposed weights. */
int ossid_conv3x3_wgrad_splits(int B, int H, int W, int Cin, int Cout);
size_t ossid_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ossid_conv3x3_wgrad(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, int in_channel_stride,
                        int dy_channel_stride, void* workspace, size_t workspace_bytes, float* dw, int accumulate,
                        void* stream);

/* D16  weight gradient of a 3x3 / pad 1 or 1x1 convolution whose INPUT carried a fused prologue in the forward pass
 * (training-mode BatchNorm folded to a per-channel affine, + ReLU: DenseNet's BN-ReLU-Conv, models/dtoid/network.py:164-184;
 * the head's `norm(F.elu(conv(x)))` feeding the next conv, :330-357):
 *   dw[co][ci][tap] (+)= sum_{b,y,x} dy[b][y][x][co] * P(x)[b][y+dy][x+dx][ci],  P(v) = relu?(v * pre_scale[ci] + pre_shift[ci])
 * on real pixels, zero outside the image (pre_scale NULL = identity). x [B][H][W][in_channel_stride], dy
 * [B][H][W][dy_channel_stride] channels-last (0 = cin / cout); dw in torch layout [cout][cin][kh][kw]. Operands are staged
 * through LDS with the pixels on K: as bf16 hi/lo images read back K-major (ds_read_b64_tr_b16) for three
 * v_mfma_f32_32x32x16_bf16 per f32 product (split-bf16, ~5e-6 of the result's scale; ossid_conv_wgrad_split_bf16() != 0),
 * or as f32 for v_mfma_f32_32x32x2_f32 (every layer of a -DOSSID_WGRAD_F32 build); split-K slabs in `workspace`
 * (ossid_conv_wgrad_workspace_bytes; workspace_bytes below it is OSSID_EINVAL), summed in a fixed order -- bit-reproducible,
 * no float atomics. cin, cout % 4 == 0. */
typedef struct ossid_wgrad_desc {
    const float* x;
    const float* dy;
    const float* pre_scale;
    const float* pre_shift;
    float* dw;
    void* workspace;
    size_t workspace_bytes;
    int32_t batch, height, width, cin, cout, taps, pre_relu, accumulate;
    int32_t in_channel_stride, dy_channel_stride;
    int32_t src_height, src_width;   /* > 0 (3x3 only): x is [B][src_h][src_w][..], nearest-neighbour up-sampled to
                                        [height][width] on the fly, as in the forward (ossid_conv_desc) */
    /* ABI 5. Optional: the output gradient is dy + dy_add_scale[co] * dy_add + dy_add_shift[co], formed while dy is staged
     * (dy_add [B][H][W][dy_channel_stride] like dy): the statistics term of a training BatchNorm's backward, dz = g + c_x y + c_1,
     * without a pass that materialises dz. Only the 1x1 problems csrc/wgrad_t9.hip takes (a dense layer's c -> 128) support it;
     * any other problem with dy_add != NULL is rejected. */
    const float* dy_add;
    const float* dy_add_scale;
    const float* dy_add_shift;
} ossid_wgrad_desc;
int ossid_conv_wgrad_split_bf16(void);
size_t ossid_conv_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int taps);
int ossid_conv_wgrad(const ossid_wgrad_desc* desc_host, void* stream);
/* Up to 48 INDEPENDENT weight gradients (e.g. the 2 x L of one DenseNet block, each too small to fill the chip) as one
 * launch per tiling variant plus one grouped slab reduction; each descriptor's `workspace` field is ignored, the slabs
 * of all problems live in the one `workspace` of ossid_conv_wgrad_group_workspace_bytes(descs, n) bytes. Problems that
 * csrc/wgrad_t9.hip takes go there in rounds -- one geometry (batch, height, width) per round, fixed by the first such
 * problem still left -- so a group may mix geometries. */
size_t ossid_conv_wgrad_group_workspace_bytes(const ossid_wgrad_desc* descs_host, int n);
int ossid_conv_wgrad_group(const ossid_wgrad_desc* descs_host, int n, void* workspace, size_t workspace_bytes, void* stream);

/* D16  packed weights of the DATA gradient: dx = conv(dy, W') with W'[ci][co][tap] = w[co][ci][taps-1-tap] (transposed,
 * rotated by 180 degrees), in the layout ossid_conv_nhwc_fwd reads for a [cout' = Cin][cin' = Cout] layer -- the data
 * gradient itself is that forward kernel on dy. Cout % 16 == 0; wpk has ossid_conv_packed_floats(Cin, Cout, taps) floats. */
int ossid_conv_pack_weights_dgrad(const float* w, int Cout, int Cin, int taps, float* wpk, void* stream);

/* D16  one generic channels-last pass of the training step (rows = B*H*W pixels, `channels` % 4 == 0):
 *     m   = 1 (mask_mode 0) | [mask_scale[c] * x + mask_shift[c] > 0] (1: ReLU behind a folded BatchNorm)
 *           | (x > 0 ? 1 : x + 1) (2: ELU'(v) written in terms of x = ELU(v)) | [x > 0] (3: ReLU'(v) in terms of x = ReLU(v))
 *     r   = (alpha[c] * g + beta[c] * x + kappa[c]) * m              (NULL alpha/beta/kappa = 1 / 0 / 0)
 *     out = r, or out + r when accumulate != 0                        (out NULL: sums only)
 *     sums[0][c], sums[1][c] = sum over rows of (g*m, g*m*x) (sum_mode 1), (r, r*x) (sum_mode 2) or, for BatchNorm batch
 *           statistics, (g - pivot[c], (g - pivot[c])^2) (sum_mode 3: sums about a per-channel pivot -- the tensor's first
 *           row -- so that a channel whose spread is small against its mean loses nothing to E[x^2] - E[x]^2; the
 *           pivot is copied to a third row sums[2][c]); 0 = none
 * Instances: BatchNorm batch statistics (g = x, sum_mode 1: sum x, sum x^2); backward of ELU + BatchNorm statistics
 * (alpha 1, beta/kappa from ossid_bn_fold_bwd, mask 2, sum_mode 2 -> the bias gradient); backward of a folded
 * BatchNorm+ReLU prologue (g = d out of the data gradient, mask 1, alpha = scale, sum_mode 1 -> d shift, d scale);
 * DenseNet's concatenation gradient (accumulate into the block's gradient buffer). Column sums go through per-block
 * partials [ossid_chan_op_partials(rows, channels)][2][channels] floats and are combined in a fixed order in double. */
typedef struct ossid_chan_op_desc {
    const float* g;
    const float* x;
    float* out;
    const float* alpha;
    const float* beta;
    const float* kappa;
    const float* mask_scale;
    const float* mask_shift;
    float* partials;
    float* sums;
    const float* pivot;              /* sum_mode 3: [channels] floats the statistics are taken about (row 0 of the tensor) */
    int64_t n_rows;
    int32_t channels, g_stride, x_stride, out_stride, mask_mode, accumulate, sum_mode;
    int32_t sums_row_stride;         /* floats between sums[0][.] and sums[1][.] (0 = channels): lets a layer write the
                                        statistics of its channel slice into a block-wide [2][C_total] table */
    int32_t defer_finalize;          /* != 0: leave the column sums as the ossid_chan_op_partials(rows, channels)
                                        per-block partials in `partials` (sums may be NULL); the consumer --
                                        ossid_bn_fold_fwd / _bwd with n_partials > 0 -- combines them itself */
} ossid_chan_op_desc;
int ossid_chan_op_partials(long long n_rows, int channels);
int ossid_chan_op(const ossid_chan_op_desc* desc_host, void* stream);

/* Zero `bytes` bytes at `ptr` on `stream` (an accumulator a recorded launch sequence must clear on every replay: the
 * coefficient table of a dense block's backward pass; replaces torch.zeros inside such a sequence). */
int ossid_fill_zero(void* ptr, size_t bytes, void* stream);

/* Replay of a recorded launch sequence. The finetune step (scripts/online_learning.py:650-679) is ~1 800 small launches
 * of fixed shape from one host thread; a binding records the launches one fixed-shape piece makes (a DenseNet block's
 * forward, a template encoder's backward: models/dtoid/network.py:160-279) ONCE, as calls of this library's own
 * stream-taking entry points with their argument values, and hands the list back here every step: the loop below re-issues
 * them with the current stream handles, so a recorded launch costs the host its hipLaunchKernel and nothing else.
 *   fn        one of this library's entry points of the form int f(..., void* stream) (every argument an integer, a
 *             pointer, a size_t, a float or a double; the stream LAST), or NULL for a stream-order op: streams[slot]
 *             waits for everything streams[wait_for] holds when the op is reached (an event owned by the op, created at
 *             its first replay; ossid_seq_release destroys it);
 *   iarg      the integer-class arguments in order, WITHOUT the stream (pointers and sign-extended integers);
 *   fparg     the floating-point arguments in order: a float's bits in the low 32, a double's in all 64;
 *   slot      index into the replay's stream table of the stream the call gets.
 * Descriptor structs a call points to (ossid_conv_desc ...) are read at every replay: they, and all device memory they
 * name, must stay alive and at the same addresses for as long as the sequence is replayed. Returns the first non-zero
 * status (failed_at_host, may be NULL, then holds the op's index; -1 after a clean replay). x86-64 System V hosts only. */
#define OSSID_SEQ_MAX_INT 24
#define OSSID_SEQ_MAX_FP 8
typedef struct ossid_seq_op {
    void* fn;
    void* event;
    int32_t slot, wait_for, n_int, n_fp;
    uint64_t iarg[OSSID_SEQ_MAX_INT];
    uint64_t fparg[OSSID_SEQ_MAX_FP];
} ossid_seq_op;
int ossid_seq_replay(ossid_seq_op* ops_host, int n, void* const* streams_host, int n_streams, int* failed_at_host);
int ossid_seq_release(ossid_seq_op* ops_host, int n);
/* Calling-convention probe for the tests of ossid_seq_replay (no device work): writes its 14 arguments and the stream
 * handle, each converted to double, to out_host[0..14]. */
int ossid_seq_probe(int32_t i0, float f0, const void* p1, double d1, int64_t l2, int32_t i3, float f2, size_t s4, int32_t i5,
                    int32_t i6, int32_t i7, double d3, int32_t i8, int64_t l9, double* out_host, void* stream);

/* Segmentation term of DtoidNet.forward's loss and its metric (models/dtoid/__init__.py:210-232) in one pass:
 *   prob = sigmoid(logit) [B][hw];  out[0] = BCELoss(prob, mask) (mean over B*hw, torch's clamps: log terms >= -100);
 *   out[1 + b] = IoU of (prob > 0.5) vs (mask > 0) of image b (0 for an empty union: pl.metrics iou(ignore_index=0));
 *   dlogit_sum [B][hw] = d(SUM of the BCE terms)/d(logit) -- the backward pass scales it by upstream / (B*hw).
 * workspace >= ossid_seg_bce_iou_workspace_bytes(B), 8-byte aligned. Deterministic (fixed-order double sums). */
size_t ossid_seg_bce_iou_workspace_bytes(int B);
int ossid_seg_bce_iou_fwd(const float* logit, const float* mask, int B, long long hw, float* prob, float* dlogit_sum,
                          float* out, void* workspace, size_t workspace_bytes, void* stream);

/* 3x3 / pad 1 convolution with ONE output channel in training -- the decoder's `seg_final` (nn.Conv2d(16, 1, 3, padding=1),
 * models/dtoid/network.py:326, :362): x [B][H][W][C] channels-last (C % 4 == 0), w [C][3][3] = the parameter's layout,
 * out / g [B][H][W]. Forward (+ bias), data gradient, weight + bias gradient (fixed-order sums through `workspace` >=
 * ossid_conv3x3_c1_wgrad_workspace_bytes()). Vector-ALU kernels: a one-row output is no matrix-core shape. */
int ossid_conv3x3_c1_fwd(const float* x, int B, int H, int W, int C, const float* w, const float* bias, float* out, void* stream);
int ossid_conv3x3_c1_dgrad(const float* g, int B, int H, int W, int C, const float* w, float* dx, void* stream);
size_t ossid_conv3x3_c1_wgrad_workspace_bytes(void);
int ossid_conv3x3_c1_wgrad(const float* x, const float* g, int B, int H, int W, int C, void* workspace, size_t workspace_bytes,
                           float* dw, float* db, void* stream);

/* Convolution weights [cout][cin][k][k] -> the [cout][kpad] matrix in ossid_im2col_stem's column order
 * ((ky * k + kx) * cin + c, zero-padded), or back (inverse = 1: a weight GRADIENT computed on the im2col columns returns to
 * the parameter's layout). The strided stems (7x7 / 2 of the image backbone, network.py:164-170; 3x3 / 2 of the template
 * encoders, :203-208) run as im2col + a 1x1 MFMA convolution. */
int ossid_stem_weight_relayout(const float* src, float* dst, int cout, int cin, int k, int kpad, int inverse, void* stream);

/* D16  training-mode BatchNorm2d (nn.BatchNorm2d in train(), online_learning.py:656) folded into the per-channel affine
 * the NEXT convolution applies while staging its input: from sums = (sum x, sum x^2) over n rows,
 *   (sums[c], sums[sums_row_stride + c]; 0 = C; taken about pivot[c] when pivot != NULL: mean = pivot + S1/n,
 *   var = S2/n - (S1/n)^2) mean, biased var -> scale = gamma * rstd, shift = beta - mean * scale; running statistics updated in place with
 *   `momentum` (unbiased variance), as torch does. Backward: (d scale, d shift) -> d gamma, d beta and the coefficients of
 *   the statistics' own gradient  dx += coef_x[c] * x + coef_1[c]  (= d mean / n + 2 (x - mean) d var / n), which the
 *   producer's ossid_chan_op pass applies (accumulate != 0: += onto coef_x / coef_1, several consumers of one tensor).
 *   n_partials > 0: the two sums (forward: sum x, sum x^2; backward: d shift, d scale) are read as the per-block partials a
 *   deferred ossid_chan_op left in `partials` and combined here, in the same fixed order. */
int ossid_bn_fold_fwd(const float* sums, int sums_row_stride, const float* partials, int n_partials, const float* pivot, int C,
                      double n, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, float* scale, float* shift, float* mean_out, float* rstd_out, void* stream);
/* ossid_bn_fold_fwd for a dense block's norm1: `table` [3][row_stride] (sums, sums of squares, pivots: what ossid_chan_op sum_mode 3
 * finalizes) is complete for the first tail_c0 channels; the last C - tail_c0 channels still are the partial rows of a DEFERRED
 * ossid_chan_op over the slab the previous layer appended (tail_partials [n_partials][2][C - tail_c0], tail_pivot = that launch's
 * pivot row): they are finalized into the table here and all C channels folded -- one launch instead of finalize + fold.
 * tail_c0 % 32 == 0. */
int ossid_bn_fold_fwd_tail(float* table, int row_stride, int tail_c0, const float* tail_partials, int n_partials,
                           const float* tail_pivot, int C, double n, const float* gamma, const float* beta, float eps, float momentum,
                           float* running_mean, float* running_var, float* scale, float* shift, float* mean_out, float* rstd_out,
                           void* stream);
/* zero_row (may be NULL): C floats set to 0 by the same launch -- the unused third row of the [3][C] gradient a caller hands
 * back for the statistics (constant term, coefficient of x, pivot: the pivot has no gradient). */
int ossid_bn_fold_bwd(const float* dscale, const float* dshift, const float* partials, int n_partials, const float* gamma,
                      const float* mean, const float* rstd, int C, double n, float* dgamma, float* dbeta, float* coef_x,
                      float* coef_1, int accumulate, float* zero_row, void* stream);

/* sums[c], sums[sums_row_stride + c] = the column sums left as n_partials partial rows [n][2][C] by ossid_chan_op
 * (defer_finalize), combined in a fixed order in double. */
int ossid_colsum_finalize(const float* partials, int n_partials, int C, float* sums, int sums_row_stride, void* stream);

/* D16  all convolution weights of a training step re-packed in ONE launch (they change every optimizer step): a device
 * table with one row per (layer, layout): kind 0 = the forward layout of ossid_conv_pack_weights, 1 = the data-gradient
 * layout of ossid_conv_pack_weights_dgrad, 2 / 3 = ossid_conv_pack_weights_wino with dgrad = 0 / 1 (taps = 9), 4 / 5 = kinds
 * 0 / 1 for exact launches (ossid_conv_desc::exact = 1), 6 / 7 = for three-way-split launches (exact = 2); first_block = prefix sum of ceil(packed float4 / 256) over the rows before. */
typedef struct ossid_pack_row {
    const float* w;
    float* wpk;
    int64_t first_block;
    int32_t cout, cin, taps, kind;
} ossid_pack_row;
int ossid_conv_pack_weights_table(const ossid_pack_row* rows_device, int n_rows, long long total_blocks, void* stream);

/* D16  backward of a dense layer's 1x1 convolution (torchvision _DenseLayer.conv1 inside ImageFeatExtract, network.py:164-184)
 * with the block's gradient accumulation fused in (csrc/dense_bwd.hip): for the first c channels of the gradient buffer G
 * [n_rows][channel_stride],  G[r][ch] += alpha[ch] * m * (dz[r][:] . W1[:, ch]),  m = (mask_scale[ch] x[r][ch] + mask_shift[ch] > 0)
 * -- the data gradient of conv1 (c -> 128; wpk_dgrad = ossid_conv_pack_weights_dgrad(w [128][c][1])) through relu(norm1(.)) --
 * and norm1's column sums as partial rows for ossid_bn_fold_bwd: partials [P][2][c], row 0 = sum of g m, row 1 = sum of g m x
 * (g = the raw data gradient), P = ossid_dense_dgrad1_acc_partials(n_rows). What ossid_conv_nhwc_fwd (data-gradient weights)
 * followed by ossid_chan_op (mask_mode 1, accumulate, sum_mode 1) computes, without the [n_rows][c] tensor in between; same
 * three-product bf16 arithmetic, f32 sums in another order. c % 32 == 0, c <= 1024, n_rows * channel_stride < 2^32; returns
 * OSSID_EINVAL in a -DOSSID_CONV_F32 build. dz_add (NULL = none): dz is dz + dz_add_scale[k] * dz_add + dz_add_shift[k], formed
 * while dz is staged (dz_add [n_rows][128]: see ossid_wgrad_desc.dy_add). */
/* ... and its FORWARD with norm2's batch statistics in the epilogue: y1 [n_rows][128] = conv1(relu(pre_scale x + pre_shift)) on
 * the first c channels of x [n_rows][channel_stride], wpk_x6 = ossid_conv_pack_weights_form(w [128][c][1], exact = 2) (the
 * three-way split: f32-level accuracy), and P = ossid_dense_fwd1_stats_partials(n_rows) partial rows [P][3][128] = per-channel
 * (sum of (y1 - p_w), sum of (y1 - p_w)^2, p_w) about each workgroup's OWN pivot p_w (its first output of the channel) with
 * counts [P] = pixels per row: ossid_conv_nhwc_fwd (exact = 2) followed by ossid_chan_op (sum_mode 3) without the second read of
 * y1. ossid_bn_fold_fwd_rows is ossid_bn_fold_fwd for such rows (moved to one common pivot in double). c % 32 == 0. */
int ossid_dense_fwd1_stats_partials(long long n_rows);
int ossid_dense_fwd1_stats(const float* x, int channel_stride, int c, const float* pre_scale, const float* pre_shift,
                           const float* wpk_x6, long long n_rows, float* y1, float* partials, float* counts, void* stream);
int ossid_bn_fold_fwd_rows(const float* partials, const float* counts, int n_partials, int C, double n, const float* gamma,
                           const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* scale,
                           float* shift, float* mean_out, float* rstd_out, void* stream);
/* ... and the layer's 3x3 data gradient (32 -> 128) with norm2 / ReLU's backward in its epilogue: db [B*H*W][128] = alpha m (g * W2'),
 * m = (mask_scale y1 + mask_shift > 0), g = the gradient of the layer's 32 channels ([B][H][W][g_channel_stride]: a channel slice),
 * wpk_dgrad = ossid_conv_pack_weights_dgrad(w2 [32][128][9]), and partial rows [P][2][128] (sum g' m, sum g' m y1, g' the raw data
 * gradient) for ossid_bn_fold_bwd, P = ossid_dense_dgrad3_mask_partials(B, H, W): ossid_conv_nhwc_fwd / ossid_conv3x3_wino_fwd on
 * the data-gradient weights followed by ossid_chan_op (mask_mode 1, sum_mode 1), without the second pass. */
int ossid_dense_dgrad3_mask_partials(int B, int H, int W);
int ossid_dense_dgrad3_mask(const float* g, int g_channel_stride, const float* wpk_dgrad, const float* y1, float* db, int B, int H,
                            int W, const float* alpha, const float* mask_scale, const float* mask_shift, float* partials,
                            void* stream);
int ossid_dense_dgrad1_acc_partials(long long n_rows);
int ossid_dense_dgrad1_acc(const float* dz, const float* wpk_dgrad, const float* x, float* G, long long n_rows, int c,
                           int channel_stride, const float* alpha, const float* mask_scale, const float* mask_shift, float* partials,
                           const float* dz_add, const float* dz_add_scale, const float* dz_add_shift, void* stream);

/* D4  nn.AvgPool2d(2, stride) of the DenseNet transitions (stride 2; the third one stride 1, network.py:165),
 * channels-last. backward != 0: x is d out [B][Ho][Wo][C] and out receives d in [B][H][W][C]. */
int ossid_avgpool2_nhwc(const float* x, int B, int H, int W, int C, int stride, float* out, int backward, void* stream);

/* D6  gradient of F.interpolate(mode="nearest") [Hs][Ws] -> [H][W] (network.py:354-357), channels-last: every source
 * pixel sums the destination pixels that read it, rows row_start[sy] .. row_start[sy+1]-1 (int32 [Hs+1], device),
 * columns likewise -- tables built by the caller with the forward's index formula. */
int ossid_upsample_nearest_bwd_nhwc(const float* dup, int B, int Hs, int Ws, int H, int W, int C, const int32_t* row_start,
                                    const int32_t* col_start, float* dsrc, void* stream);

/* D15  DetectionLoss.forward (models/dtoid/loss.py:46-175) and its gradient in three launches: focal classification
 * loss (alpha, gamma) with IoU anchor assignment (>= 0.5 positive, < 0.4 negative, else ignored; probabilities clamped to
 * [1e-4, 1 - 1e-4]) + smooth-L1 (beta 1/9) box regression on the positives against the encoded assigned box
 * ((dx, dy) / 0.1, (log dw, log dh) / 0.2), per image normalised by #positives (x 4), averaged over the batch.
 * cls [B][A][C] probabilities, reg [B][A][4], anchors [A][4], annotations [B][G][5] (x1,y1,x2,y2,label; label -1 = padding;
 * G <= 16). fwd writes losses2 = (cls_loss, reg_loss), the un-normalised gradients dcls_raw / dreg_raw (same shapes as
 * cls / reg) and scales2B [2][B]; bwd: dcls = grad_losses2[0] * scales[0][b] * dcls_raw, dreg likewise (grad_losses2 =
 * the upstream gradient of the two losses, device). workspace: ossid_focal_smoothl1_loss_workspace_floats(B, A) floats.
 * Sums are formed in a fixed order (per-block partials, one wave per image): bit-reproducible. */
size_t ossid_focal_smoothl1_loss_workspace_floats(int B, int A);
int ossid_focal_smoothl1_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* annotations, int B,
                                  int A, int C, int G, float alpha, float gamma, float* dcls_raw, float* dreg_raw,
                                  float* workspace, float* losses2, float* scales2B, void* stream);
int ossid_focal_smoothl1_loss_bwd(const float* dcls_raw, const float* dreg_raw, const float* scales2B, const float* grad_losses2,
                                  int B, int A, int C, float* dcls, float* dreg, void* stream);

/* D1-D4  the strided stems of the two backbones (too few input channels for the MFMA convolution's channel tiling) as
 * im2col + a 1x1 convolution on ossid_conv_nhwc_fwd: out [B][Ho][Wo][Kpad] channels-last, column (ky*k + kx)*Cin + ci =
 * normalised img[b][ci][yo*stride - pad + ky][xo*stride - pad + kx] (0 outside the image and in the columns past
 * k*k*Cin); img is NCHW as the caller holds it; mean / inv_std [Cin] (device, NULL = none) = normalizeImageRange
 * (utils/__init__.py:33-39) applied to real pixels on the way. DenseNet conv0 (network.py:164): k 7, stride 2, pad 3,
 * Kpad 160; SqueezeNet stem (:203-208): k 3, stride 2, pad 0, Kpad 48. The host re-lays the conv weight [Cout][Cin][k][k] to
 * [Cout][Kpad] in the same column order. */
int ossid_im2col_stem(const float* img_nchw, int B, int Cin, int H, int W, int k, int stride, int pad, int Kpad,
                      const float* mean, const float* inv_std, float* out, void* stream);
/* D6  the small remainders of the correlation head, deterministic (fixed-order sums):
 * ossid_conv1x1_c1_fwd: nn.Conv2d(C, 1, 1) on channels-last x [rows][C] (`corr_conv_heatmap`, network.py:334, :349):
 *   out[r] = sum_c w[c] x[r][c] + bias[0], through a sigmoid when sigmoid != 0 (heat_map = torch.sigmoid(...)); C % 4 == 0.
 * ossid_conv1x1_c1_bwd: dx[r][c] = g[r] w[c] (dx may be NULL), dw_db [C + 1] = (sum_r g[r] x[r][c], sum_r g[r]); C / 4 a power
 *   of two <= 256; workspace >= ossid_conv1x1_c1_bwd_workspace_floats(rows, C) floats.
 * ossid_spatial_mean: F.avg_pool2d(x, full window) (`avg_pool2d(template_feat, 7)`, network.py:343): x [B][C][HW] (NCHW) or
 *   [B][HW][C] (channels_last != 0) -> out [B][C]; backward != 0: x = g [B][C] -> out = g / HW broadcast in x's layout.
 * ossid_small_matmul: out [M][N] = a [M][K] b [K][N] (row-major, M <= 65535: a handful of rows against a wide matrix). */
int ossid_conv1x1_c1_fwd(const float* x, long long rows, int C, const float* w, const float* bias, int sigmoid, float* out,
                         void* stream);
size_t ossid_conv1x1_c1_bwd_workspace_floats(long long rows, int C);
int ossid_conv1x1_c1_bwd(const float* x, const float* g, long long rows, int C, const float* w, float* workspace, float* dx,
                         float* dw_db, void* stream);
int ossid_spatial_mean(const float* x, int B, int HW, int C, int channels_last, int backward, float* out, void* stream);
int ossid_small_matmul(const float* a, const float* b, int M, int K, int N, float* out, void* stream);

/* D4  a DenseNet block of ImageFeatExtract at TEST time with one launch per layer (csrc/dense.hip; network.py:164-184 builds
 * torchvision's densenet121: each _DenseLayer is norm1 -> ReLU -> conv1 1x1 (c -> 128) -> norm2 -> ReLU -> conv2 3x3
 * (128 -> 32) on the concatenation of everything before it; eval mode, BatchNorms as per-channel scale / shift).
 * The 1x1 is linear in its input channels, so the bottleneck sums y [L][pixels][128] of ALL layers are kept up to date
 * incrementally: ossid_dense_entry writes every layer's share of the block's c0 input channels, and ossid_dense_layer(l)
 * runs layer l's 3x3 on relu(norm2(y[l])), appends its 32 channels to buf [B][H][W][ctot] at channel c0 + 32 l, and adds
 * their share to y[m] for every later layer m. Same values as ossid_conv_nhwc_fwd per layer up to the order of the f32
 * summation (same three-product bf16 arithmetic, same packed weights).
 * table: device array of nlayers records {const float* w1pk; const float* s1; const float* t1; int64 units} (32 bytes each,
 * ossid_dense_table_bytes): conv1 packed by ossid_conv_pack_weights(w [128][c_m][1]), norm1 as scale / shift [c_m],
 * units = c_m / 16 with c_m = c0 + 32 m. w2pk = ossid_conv_pack_weights(conv2.weight [32][128][9]); s2 / t2 [128] = norm2.
 * c0 in {64, 128, 256, 512}; growth 32 and bottleneck 128 are fixed. ossid_dense_fused_available() = 0 in a
 * -DOSSID_CONV_F32 build (no split form): both entries then return OSSID_EINVAL and the caller keeps the per-layer path. */
int ossid_dense_fused_available(void);
size_t ossid_dense_table_bytes(int nlayers);
int ossid_dense_entry(const float* buf, int ctot, int c0, long long pixels, int nlayers, const void* table, float* y, void* stream);
int ossid_dense_layer(float* y, float* buf, int B, int H, int W, int ctot, int c0, int layer, int nlayers, const float* w2pk,
                      const float* s2, const float* t2, const void* table, void* stream);

/* D4  DenseNet-121 conv0 = nn.Conv2d(3, 64, 7, stride 2, padding 3) of ImageFeatExtract (network.py:164-170, :175-177) as an
 * IMPLICIT-im2col convolution on the f32 matrix cores (csrc/stem.hip; exact f32: an fmaf chain), and its weight gradient
 * (the image is an input: there is no data gradient). img NCHW [B][3][H][W] as the caller holds it; mean / inv_std [3]
 * (device, NULL = none) = normalizeImageRange (utils/__init__.py:33-39) applied to real pixels while staging, zero padding
 * in normalised space as the reference has it; weight / dweight [64][3][7][7] = the parameter's own layout (no packing);
 * out / dy [B][Ho][Wo][64] channels-last, Ho = (H - 1) / 2 + 1; bias [64] or NULL. Only this geometry is accepted
 * (Cin 3, Cout 64, k 7, stride 2, pad 3): anything else returns OSSID_EINVAL. The weight gradient sums per-workgroup
 * partial slabs in a fixed order (bit-reproducible); workspace >= ossid_stem_conv_wgrad_workspace_bytes(B, H, W), 16-byte
 * aligned; accumulate != 0 adds to dweight. */
int ossid_stem_conv_fwd(const float* img_nchw, int B, int Cin, int H, int W, const float* weight, int Cout, int k, int stride,
                        int pad, const float* bias, const float* mean, const float* inv_std, float* out, void* stream);
size_t ossid_stem_conv_wgrad_workspace_bytes(int B, int H, int W);
int ossid_stem_conv_wgrad(const float* img_nchw, const float* dy, int B, int Cin, int H, int W, int Cout, int k, int stride,
                          int pad, const float* mean, const float* inv_std, void* workspace, size_t workspace_bytes,
                          float* dweight, int accumulate, void* stream);
/* D4  relu(scale[c] * (x0 + conv2d_dw_group(x0, kernels)) + shift[c]) (network.py:178-181: the global-template modulation
 * of the stem output, norm0 in eval mode, relu0), channels-last; kernels [B or 1][C][3][3], kernels_batch_stride = C*9 or
 * 0 (one kernel set for the whole batch). */
int ossid_stem_tail_nhwc(const float* x0, const float* kernels, int kernels_batch_stride, const float* scale, const float* shift,
                         int B, int H, int W, int C, float* out, void* stream);
/* D4 at test time, fused further: ossid_stem_tail_pool_nhwc = ossid_stem_tail_nhwc followed by pool0 = nn.MaxPool2d(3, 2, 1)
 * (network.py:170-179) in one pass, written into the first C channels of a buffer with out_channel_stride floats per pixel (the
 * dense block's resident buffer): out [B][Ho][Wo][out_channel_stride], Ho = (H - 1) / 2 + 1.
 * ossid_bn_relu_avgpool2_nhwc: relu(scale * x + shift) averaged over 2 x 2 windows (stride 1 or 2) -- the front of a DenseNet
 * transition (norm -> relu -> conv 1x1 -> AvgPool2d) with the pool moved in front of the bias-free 1x1 convolution, with which
 * it commutes: x [B][H][W][in_channel_stride] (first C channels) -> out [B][Ho][Wo][C]. */
int ossid_stem_tail_pool_nhwc(const float* x0, const float* kernels, int kernels_batch_stride, const float* scale, const float* shift,
                              int B, int H, int W, int C, float* out, int out_channel_stride, void* stream);
int ossid_bn_relu_avgpool2_nhwc(const float* x, int B, int H, int W, int C, int in_channel_stride, const float* scale,
                                const float* shift, int stride, float* out, void* stream);
/* D2-D4  nn.MaxPool2d(k, stride, padding, ceil_mode) channels-last (DenseNet pool0: 3, 2, 1; SqueezeNet: 3, 2, 0, ceil). */
int ossid_maxpool_nhwc(const float* x, int B, int H, int W, int C, int k, int stride, int pad, int ceil_mode, float* out,
                       void* stream);

/* Separable linear resampling of a channels-last image by tap tables (training path of the template encoders,
 * models/dtoid/network.py:223-239, :265-279):
 *   out[b][oy][ox][out_channel_offset + c] = sum_{i,j < T} wy[oy][i] wx[ox][j] x[b][iy[oy][i]][ix[ox][j]][c]
 * taps_*_idx [n_out][T] int32 (-1 = unused tap), taps_*_w [n_out][T] float32, T <= 8; channel strides in floats (0 = C).
 * Covers F.interpolate(mode="bilinear", align_corners=False) (T = 2), its adjoint (transposed tables), the crop that
 * turns a padded 3x3 convolution into the reference's valid one (T = 1) and the crop's adjoint (zero padding). */
int ossid_resample_taps_nhwc(const float* x, int B, int Hin, int Win, int C, int x_channel_stride, int Hout, int Wout,
                             const int32_t* taps_y_idx, const float* taps_y_w, const int32_t* taps_x_idx, const float* taps_x_w,
                             int T, float* out, int out_channel_stride, int out_channel_offset, void* stream);

/* D16  training-side companions of the stem kernels (finetune step, channels-last):
 * ossid_dw_add_nhwc: out = x + conv2d_dw_group(x, kernels) (network.py:178-179), flip != 0: the taps rotated by 180 degrees
 *   (= the gradient with respect to x of the same expression applied to the upstream gradient);
 * ossid_dw_bwd_k_nhwc: dk[b][c][ky][kx] = sum_px g[b][px][c] * x[b][px + tap][c] (gradient with respect to the per-sample
 *   kernels), per-row-chunk partials in `workspace` (ossid_dw_bwd_k_workspace_floats), summed in a fixed order;
 * ossid_maxpool_idx_nhwc / ossid_maxpool_bwd_nhwc: nn.MaxPool2d forward that also stores the window position of the
 *   maximum (uint8, first maximum in (ky, kx) order, as torch) and the backward as a gather over the windows containing
 *   each input pixel -- no atomics. */
int ossid_dw_add_nhwc(const float* x, const float* kernels, int kernels_batch_stride, int B, int H, int W, int C, int flip,
                      float* out, void* stream);
/* ossid_dw_add_nhwc that also leaves the column sums of its OUTPUT y about pivot[c] = y[0][0][0][c] -- (sum (y - pivot),
 * sum (y - pivot)^2), the batch statistics of the BatchNorm that follows (norm0) -- as ossid_dw_add_stats_partials(B, H, W, C)
 * partial rows [P][2][C] for ossid_bn_fold_fwd (n_partials = P, pivot = pivot_out [C]): the statistics cost no pass of
 * their own. C / 4 must be a power of two <= 64 (these four entry points). partials / pivot_out both NULL: no statistics. */
int ossid_dw_add_stats_partials(int B, int H, int W, int C);
int ossid_dw_add_stats_nhwc(const float* x, const float* kernels, int kernels_batch_stride, int B, int H, int W, int C, int flip,
                            float* out, float* partials, float* pivot_out, void* stream);
/* D4  norm0 + relu0 + pool0 of the training stem without ever writing the normalised tensor (network.py:180-181 with
 * torchvision's MaxPool2d(3, 2, 1)):  out [B][Ho][Wo][C] = maxpool(relu(scale[c] * m + shift[c])), argmax = the window
 * position (ky * 3 + kx, uint8) of the first maximum, Ho = (H - 1) / 2 + 1.
 * Backward in two passes over m, the un-pooled gradient gm = [scale m + shift > 0] * (sum of dpooled whose maximum sat at
 * this pixel) formed on the fly both times: dm == NULL: (sum gm, sum gm * m) -> ossid_stem_pool_bwd_partials(B, H, W, C)
 * partial rows [P][2][C] floats for ossid_bn_fold_bwd; partials == NULL: dm = scale gm + coef_x m + coef_1 (coefficients from that fold). */
int ossid_stem_pool_fwd(const float* m, const float* scale, const float* shift, int B, int H, int W, int C, float* out,
                        uint8_t* argmax, void* stream);
int ossid_stem_pool_bwd_partials(int B, int H, int W, int C);
int ossid_stem_pool_bwd(const float* m, const uint8_t* argmax, const float* dpooled, const float* scale, const float* shift,
                        const float* coef_x, const float* coef_1, int B, int H, int W, int C, float* partials, float* dm,
                        void* stream);
size_t ossid_dw_bwd_k_workspace_floats(int B, int H, int W, int C);
int ossid_dw_bwd_k_nhwc(const float* x, const float* g, int B, int H, int W, int C, float* workspace, float* dk, void* stream);
int ossid_maxpool_idx_nhwc(const float* x, int B, int H, int W, int C, int k, int stride, int pad, int ceil_mode, float* out,
                           uint8_t* argmax, void* stream);
int ossid_maxpool_bwd_nhwc(const float* dout, const uint8_t* argmax, int B, int H, int W, int C, int k, int stride, int pad, int Ho,
                           int Wo, float* dx, void* stream);

/* D12  torch.topk(scores, k) (network.py:555: the 1000 best of the ~570 k (template, anchor) object scores of a frame):
 * values [k] in decreasing order and their int64 indices; equal scores are ordered (and, at the cut, chosen) by increasing
 * index. Radix select (three histogram passes) + ordered gather + one-workgroup sort of the k survivors; k <= 2048.
 * NaN scores order above +inf. workspace: ossid_topk_workspace_bytes(n, k) bytes. */
size_t ossid_topk_workspace_bytes(int n, int k);
int ossid_topk(const float* scores, int n, int k, void* workspace, size_t workspace_bytes, float* values, long long* indices,
               void* stream);

/* D12  torchvision.ops.nms(boxes, scores, iou_threshold)      network.py:563, models/dtoid/utils.py:33
 * boxes [n][4] (x1,y1,x2,y2) ALREADY sorted by descending score (network.py:555 feeds it the top-k order);
 * keep [n] receives the indices of the survivors in that order, *num_keep their count. n <= 16384. */
size_t ossid_nms_workspace_bytes(int n);
int ossid_nms(const float* boxes, int n, float iou_threshold, void* workspace, size_t workspace_bytes,
              int32_t* keep, int32_t* num_keep, void* stream);

/* D12  the post-processing of a frame as launches only (network.py:543-566: decode + clip, top-k of the object scores over all
 * templates, NMS), so that it can live in the frame's captured graph: scores = the object column of the class probabilities
 * (element i at scores[i * score_stride], n = templates * A of them, i = template * A + anchor), anchors [A][4], deltas [n][4].
 * Out: the k best scores in decreasing order (ties by increasing index, as ossid_topk), their indices, their decoded and
 * clipped boxes (the arithmetic of ossid_decode_clip_boxes, applied to the k survivors only), and ossid_nms's keep list over
 * them with its count. k <= 2048, n % A == 0. Nothing is read back by the host.
 * ossid_detect_emit then writes the detection list for the first `count` kept candidates (network.py:566-581; the host knows
 * count = min(*num_keep, topk) by then): row j = candidate keep[j]: score, box, index of the template that fired (as float,
 * network.py:561), that template's row of seg [templates][seg_row_floats] -- through a sigmoid when seg_sigmoid != 0
 * (models/dtoid/__init__.py:147) -- and of heat [templates][heat_row_floats]. */
size_t ossid_detect_post_workspace_bytes(int n, int k);
int ossid_detect_post(const float* scores, int n, int score_stride, int k, const float* anchors, const float* deltas, int A,
                      float img_w, float img_h, float iou_threshold, void* workspace, size_t workspace_bytes, float* out_scores,
                      long long* out_indices, float* out_boxes, int32_t* keep, int32_t* num_keep, void* stream);
int ossid_detect_emit(const float* scores, const long long* indices, const float* boxes, const int32_t* keep, int count, int A,
                      const float* seg, long long seg_row_floats, const float* heat, long long heat_row_floats, int seg_sigmoid,
                      float* out_scores, float* out_boxes, float* out_obj, float* out_seg, float* out_heat, void* stream);

/* D6  `norm(F.elu(conv(image_feat - avg_t)))` (network.py:346) for ONE image against all templates without a convolution
 * per template: conv is linear, so conv(x - a_t) = conv(x) - conv(a_t). S [H][W][channels] = conv(x) + bias, computed
 * once per frame; csub [templates][9][channels] = the response to the per-channel constant image a_t for each of the 9
 * border patterns p = 3*rowclass + colclass (class 0: first row/column, 1: interior, 2: last), one small GEMM per object.
 * out[t][y][x][out_channel_offset + o] = post(ELU(S[y][x][o] - csub[t][p(y,x)][o])). H, W >= 2; channels % 4 == 0. */
int ossid_bcast_sub_epilogue(const float* S, const float* csub, int templates, int H, int W, int channels,
                             const float* post_scale, const float* post_shift, float* out, int out_channel_stride,
                             int out_channel_offset, void* stream);

/* D6  `conv(image_feat * avg_t)` (network.py:345) with the channel contraction last, for MANY templates against one image:
 * ossid_dot_expand builds G[c][y][x][o] = sum_taps w[o][c][tap] * x[y+dy][x+dx][c] (zero padding) from the channels-last
 * image x [H][W][channels] and the weights re-laid as w_cto [channels][9][cout]; the caller then contracts
 * z[t][(y,x,o)] = sum_c avg_t[c] * G[c][(y,x,o)] with a library GEMM and finishes with ossid_bias_elu_affine_slice:
 * out[r][out_channel_offset + o] = post(ELU(z[r][o] + bias[o])), rows r = (template, pixel). cout % 4 == 0,
 * 256 % (cout/4) == 0. G is channels * H * W * cout floats (0.74 GB for 640 x 29 x 39 x 256): caller-owned. */
int ossid_dot_expand(const float* x, const float* w_cto, int channels, int cout, int H, int W, float* G, void* stream);
int ossid_bias_elu_affine_slice(const float* z, long long rows, int channels, const float* bias, const float* post_scale,
                                const float* post_shift, float* out, int out_channel_stride, int out_channel_offset,
                                void* stream);

/* D12/D13  out[j][:] = src[idx[j]][:] for j < k, rows of row_floats (% 4 == 0) floats, with sigmoid applied on the way
 * when apply_sigmoid != 0: the per-detection segmentation maps gathered from the per-template ones
 * (network.py:575-579) + `torch.sigmoid(seg)` (models/dtoid/__init__.py:147) in one pass. idx: int64, each in
 * [0, n_src_rows) (caller-checked). */
int ossid_gather_rows(const float* src, int n_src_rows, long long row_floats, const long long* idx, int k,
                      int apply_sigmoid, float* out, void* stream);

/* D10  BBoxTransform.forward + ClipBoxes.forward      network.py:42-70, :78-88
 * anchors [A][4] (shared by all rows), deltas [rows][A][4] -> boxes [rows][A][4]; std (.1,.1,.2,.2), mean 0. */
int ossid_decode_clip_boxes(const float* anchors, const float* deltas, int rows, int A, float img_w, float img_h,
                            float* boxes, void* stream);

/* D16  torch.optim.Adam(lr, weight_decay, amsgrad=True).step()      scripts/online_learning.py:258-263, :672
 * one launch over flat float buffers of n elements (n % 4 == 0); `step` is the 1-based update count. */
int ossid_amsgrad_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                       size_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                       void* stream);

/* =============================================================================================
 * The steps either side of the hot path, one frame at a time, all on the device
 * ============================================================================================= */

/* 8f-1  DTOID batch producer: processData (utils/data.py:7-83: depth2xyz at the original resolution, bilinear resize of
 * image / mask / xyz to [H][W], image /255, CHW), datasets/dtoid_bop_dataset.py:256-290.
 * img u8 [Ho][Wo][3], depth f32 [Ho][Wo] (m), mask f32 [Ho][Wo] in [0,1] -> img_out [3][H][W], xyz_out [3][H][W], mask_out [H][W].
 * Equal sizes (480x640 LM-O / YCB-V frames) are an exact copy. */
int ossid_dtoid_prep_sample(const uint8_t* img, const float* depth, const float* mask, int Ho, int Wo, float fx, float fy,
                            float cx, float cy, int H, int W, float* img_out, float* xyz_out, float* mask_out, void* stream);
/* mask -> bbox_gt (x1,y1,x2,y2,label) = min/max of the non-zero pixels (dtoid_bop_dataset.py:274-279; label -1 for an
 * empty mask) and the Gaussian heat map around its centre, float64 (utils/__init__.py:354-367; :283-287). */
int ossid_mask_bbox_heatmap(const float* mask, int H, int W, int heat_h, int heat_w, double heat_scale, double sigma,
                            int32_t* bbox5, double* heatmap, void* stream);

/* 8f-3  post-score step (scripts/online_learning.py:485-500, :557-558): a depth-only point-splat renderer in place of
 * pyrender (z-buffer of the posed model cloud, (2*radius+1)^2 pixel splats; zbuf_workspace = H*W*4 bytes), the bop19
 * visibility mask visib = (d_pred - d_obs <= delta or d_obs == 0) and d_pred > 0, and the set sizes of both IoUs:
 * counts4 = |pred&gt|, |pred|gt|, |visib&gt_visib|, |visib|gt_visib| (gt masks u8, may be NULL). */
int ossid_render_depth_points(const float* transform, const float* points, int M, float fx, float fy, float cx, float cy,
                              int H, int W, int radius, void* zbuf_workspace, float* depth_out, void* stream);
int ossid_visib_mask_iou(const float* depth_obs, const float* depth_pred, const uint8_t* gt_mask, const uint8_t* gt_mask_visib,
                         int H, int W, float delta, uint8_t* pred_mask, uint8_t* pred_mask_visib, int32_t* counts4,
                         void* stream);

/* 8f-4  ICP refinement of the chosen pose (scripts/online_learning.py:471-480: zephyr.utils.icp.icpRefinement with
 * inpaint_depth=False, icp_max_dist=0.01), point-to-point, SPEC.md section 5. One workgroup per pose, all iterations in
 * the one launch. depth f32 [H][W] (m, 0 = invalid), uv int32 [K][M][2] (x = column, y = row, (-1,-1) = no projection),
 * poses_in f64 [K][4][4], points f32 [M][3] (1 <= M <= OSSID_ICP_MAX_POINTS) -> poses_out f64 [K][4][4], fitness /
 * rmse f64 [K] of the returned pose, iterations int32 [K] (updates done). The caller owns all memory; there is no
 * workspace. Every output is written by the kernel. */
#define OSSID_ICP_MAX_POINTS 2048
int ossid_icp_refine(const float* depth, int H, int W, const int32_t* uv, const double* poses_in, const float* points, int K,
                     int M, float fx, float fy, float cx, float cy, float max_dist, int max_iter, double* poses_out,
                     double* fitness, double* rmse, int32_t* iterations, void* stream);

/* 8f-5  Point-pair-feature pose hypotheses (scripts/online_learning.py:295-301 PPFModel(...) and :413-418 / :441-447
 * find_surface_model: MVTec Halcon in the reference), SPEC.md section 6. Raw device pointers, caller-owned memory; counts
 * that depend on the data stay on the device (int32 `count`), so one frame is one launch chain with no host round trip.
 *
 * ossid_ppf_sample: voxel subsampling (SPEC 6.2) of either an f32 cloud points [N][3] (normals [N][3] for a model: then
 * a vertex needs a finite non-zero normal, nrm_out receives it normalised; without normals it is a scene point and needs
 * z > 0), or a depth image f32 [H][W] + mask u8 [H][W] (pixel i valid iff mask && depth > 0, back-projected as SPEC 5.2,
 * input index = row-major pixel index). Voxel edge h = rel * (diam > 0 ? diam : this cloud's own diameter D). Outputs:
 * idx_out int32 [max_out] (input indices, ascending), pts_out f32 [max_out][3], count[0] = the number of voxels, which
 * may exceed max_out (then only max_out rows are written; rows past min(count, max_out) are never written), stats f32 [8] =
 * lo[3], hi[3], D, h. Without a valid point lo = hi = 0, D = 0 and count = 0. With h = 0 (diam <= 0 and a cloud whose box is
 * a single point, so D = 0) nothing is kept: count = 0, stats still holds the box. */
#define OSSID_PPF_MAX_MODEL_POINTS 4096
#define OSSID_PPF_MAX_SCENE_SAMPLES 8192
size_t ossid_ppf_sample_workspace_bytes(int n_in);
int ossid_ppf_sample(const float* points, const float* normals, int N, const float* depth, const uint8_t* mask, int H, int W,
                     float fx, float fy, float cx, float cy, float rel, float diam, int max_out, void* workspace,
                     size_t workspace_bytes, int32_t* idx_out, float* pts_out, float* nrm_out, int32_t* count,
                     float* stats, void* stream);
/* The model's hash table (SPEC 6.5): Ms <= OSSID_PPF_MAX_MODEL_POINTS sampled points / unit normals, its h and D ->
 * offsets u32 [words] (words = ossid_ppf_model_table_words(...), 0 = bad arguments; offsets[(key * chunks + chunk)] ..
 * [.. + 1] delimit the entries of a key whose reference point lies in chunk = m_r / 1024), entries u32 [max_entries >=
 * Ms (Ms - 1)] = m_r * 32 + rotation bin, in unspecified order within a range. Workspace: 4 * words bytes. */
int64_t ossid_ppf_model_table_words(int Ms, float h, float D);
int ossid_ppf_model_table(const float* points, const float* normals, int Ms, float h, float D, uint32_t* offsets,
                          uint32_t* entries, int64_t max_entries, void* workspace, size_t workspace_bytes, void* stream);
/* Scene normals (SPEC 6.3) of the first min(count, cap) sampled points f32 [cap][3] (cap <= OSSID_PPF_MAX_SCENE_SAMPLES;
 * count > cap: nothing is valid): normals f32 [cap][3], ok u8 [cap] (0 = fewer than 3 neighbours within radius). */
int ossid_ppf_scene_normals(const float* scene, const int32_t* count, int cap, float radius, float* normals, uint8_t* ok,
                            void* stream);
/* Voting (SPEC 6.5) for reference points 0, ref_step, 2 ref_step, ... -> peaks int32 [max_ref][3] = (m_r, alpha, votes;
 * votes 0 = no candidate), cand_poses f64 [max_ref][4][4], max_ref = ceil(cap / ref_step). */
size_t ossid_ppf_vote_workspace_bytes(int cap, int ref_step, int Ms);
int ossid_ppf_vote(const float* scene, const float* scene_normals, const uint8_t* scene_ok, const int32_t* count, int cap,
                   int ref_step, const float* model_points, const float* model_normals, int Ms, float h, float D,
                   const uint32_t* offsets, const uint32_t* entries, void* workspace, size_t workspace_bytes,
                   int32_t* peaks, double* cand_poses, void* stream);
/* Clustering (SPEC 6.6) -> poses_out f64 [num_result][4][4], scores_out f64 [num_result] (rows past info[0] are zero),
 * info int32 [4] = results, sampled scene points (count[0]; > cap means the scene was not processed), candidates,
 * clusters. */
int ossid_ppf_cluster(const int32_t* peaks, const double* cand_poses, const int32_t* count, int cap, int ref_step, int Ms,
                      float D, float dist_rel, int num_result, double* poses_out, double* scores_out, int32_t* info,
                      void* stream);

/* Dense pose refinement of PPF hypotheses (SPEC 6.9; Halcon's DensePoseRefinement 'true', the default of the LM-O call
 * :441-447): point-to-plane Gauss-Newton of every hypothesis against a voxel sampling of the scene (ossid_ppf_sample with
 * rel = RefineSamplingRel and diam = the model's D), correspondences scene -> model. h is the refinement sampling step
 * h_r = f32(RefineSamplingRel) * D, steps <= 16. Step k accepts pairs within thr_k = f32(max(0.1 * 2^-k * D, 2 h)).
 *
 * The model grid, once per model: the Mr <= OSSID_PPF_MAX_REFINE_MODEL_POINTS refinement points f32 [Mr][3] and unit
 * normals f32 [Mr][3] (ossid_ppf_sample of the model with rel = RefineSamplingRel) -> grid, an opaque buffer of
 * ossid_ppf_refine_grid_bytes(Mr, steps, D, h) bytes (0 = bad arguments), for refinements of at most `steps` steps.
 *
 * ossid_ppf_refine, per frame: scene f32 [cap][3] with count[0] sampled points (cap <= OSSID_PPF_MAX_REFINE_SCENE_POINTS;
 * count > cap: refinement is skipped), poses_in f64 [num_poses][4][4] of which the first min(num_hyp[0], num_poses) are
 * refined (num_hyp: info[0] of ossid_ppf_cluster, read on the device) -> sorted by score descending, ties by input rank:
 * poses_out f64 [num_poses][4][4], scores f64 [num_poses] (pairs / Mr), pairs int32 [num_poses] (scene points within
 * thr_{steps-1} of the model at the final pose), steps_done int32 [num_poses]; rows past the refined ones are zero.
 * status int32 [4] = (1 if the scene was over cap else 0, count[0], hypotheses refined, 0). num_poses <= 4096.
 *
 * ossid_ppf_refine_match: the correspondence set of step `step` at each of num_poses poses (no update): match int32
 * [num_poses][cap], entry i = the matched model index of scene point i or -1, for i < count[0]. */
#define OSSID_PPF_MAX_REFINE_MODEL_POINTS 16384
#define OSSID_PPF_MAX_REFINE_SCENE_POINTS 65536
size_t ossid_ppf_refine_grid_bytes(int Mr, int steps, float D, float h);
int ossid_ppf_refine_model_grid(const float* points, const float* normals, int Mr, int steps, float D, float h, void* grid,
                                size_t grid_bytes, void* stream);
size_t ossid_ppf_refine_workspace_bytes(int cap, int num_poses);
int ossid_ppf_refine(const float* scene, const int32_t* count, int cap, const void* grid, size_t grid_bytes, int Mr,
                     const double* poses_in, const int32_t* num_hyp, int num_poses, int steps, float D, float h,
                     void* workspace, size_t workspace_bytes, double* poses_out, double* scores, int32_t* pairs,
                     int32_t* steps_done, int32_t* status, void* stream);
int ossid_ppf_refine_match(const float* scene, const int32_t* count, int cap, const void* grid, size_t grid_bytes, int Mr,
                           const double* poses, int num_poses, int steps, int step, float D, float h, void* workspace,
                           size_t workspace_bytes, int32_t* match, void* stream);

/* 8f-3b  the mesh renderer of the per-frame loop (scripts/online_learning.py:485-493: zephyr.utils.renderer.Renderer --
 * addObject(obj_id, ply_path, pose, mm2m=True), obj_nodes[obj_id].matrix = pred_pose, render(depth_only=True); pyrender's
 * rasterisation of the triangle mesh), depth only, SPEC.md section 7 (csrc/raster.hip). vertices f32 [V][3] in the units
 * of the poses' translations, faces int32 [F][3] (indices in [0, V): the caller checks them; a triangle with an index
 * outside is dropped and counted as unusable), transforms f32 [N][4][4] row-major, pixel_offset in [0, 1] (the sample of
 * pixel (x, y) is (x + pixel_offset, y + pixel_offset): 0.5 = OpenGL / pyrender, 0 = depth2xyz of this library),
 * z_near >= 0 -> depth_out f32 [N][H][W]: camera-space Z of the nearest surface, 0 where nothing is drawn. depth_out
 * doubles as the z-buffer; the workspace (16-byte aligned, ossid_raster_workspace_bytes(V, F, N) bytes, 0 = bad
 * arguments) holds the projected vertices. stats int32 [N][4] (may be NULL) = per pose: triangles dropped for an
 * unusable vertex, degenerate triangles, triangles that covered at least one sample, triangles walked by a whole wave
 * (diagnostic). F = 0 is legal (an all-zero image). Three launches, nothing read back, capturable. */
#define OSSID_RASTER_MAX_VERTICES 4194304
#define OSSID_RASTER_MAX_FACES 4194304
#define OSSID_RASTER_MAX_POSES 256
#define OSSID_RASTER_MAX_PIXELS 16777216
size_t ossid_raster_workspace_bytes(int V, int F, int N);
int ossid_raster_depth(const float* vertices, int V, const int32_t* faces, int F, const float* transforms, int N, float fx,
                       float fy, float cx, float cy, int H, int W, float pixel_offset, float z_near, void* workspace,
                       size_t workspace_bytes, float* depth_out, int32_t* stats, void* stream);

/* 8f-3c  templates from a vertex-coloured mesh, in place of the offline Blender renders the reference cuts out in
 * datasets/render_dataset.py:251-331 (processRenderGrid: mask -> square box padded 1.1x, image * mask, resized) and loads
 * in datasets/template_dataset.py:60-117. SPEC.md 7.11-7.14 (csrc/raster.hip).
 * ossid_raster_color: ossid_raster_depth's inputs plus colors u8 [V][3] (RGB) and one camera per pose, intrinsics
 * f32 [N][4] = fx, fy, cx, cy. The workspace (16-byte aligned, ossid_raster_color_workspace_bytes(V, F, N, H, W) bytes,
 * 0 = bad arguments) holds the projected vertices and one 64-bit visibility key per (pose, pixel):
 * bits(z) << 32 | face index, reduced by a minimum -- the nearest depth and, among equal depths, the lowest index of
 * `faces`. -> color_out u8 [N][H][W][3] (perspective-correct, unlit, 0 where nothing is drawn), depth_out f32 [N][H][W]
 * (bit-equal to ossid_raster_depth's when all poses share one camera), face_id_out int32 [N][H][W] (may be NULL; the
 * winner, -1 where nothing is drawn), stats as ossid_raster_depth. Three launches, nothing read back, capturable.
 * ossid_template_reduce: the exact s x s box filter over such renders at S = s T: color u8 [N][S][S][3],
 * depth f32 [N][S][S] -> img_out f32 [N][3][T][T] = ((sum of covered colours + s*s/2) / (s*s)) / 255 (integer division),
 * mask_out f32 [N][1][T][T] = covered samples / (s*s). 1 <= s <= 8, 1 <= T <= 512, 1 <= N <= OSSID_RASTER_MAX_POSES. */
size_t ossid_raster_color_workspace_bytes(int V, int F, int N, int H, int W);
int ossid_raster_color(const float* vertices, int V, const int32_t* faces, int F, const uint8_t* colors,
                       const float* transforms, int N, const float* intrinsics, int H, int W, float pixel_offset, float z_near,
                       void* workspace, size_t workspace_bytes, uint8_t* color_out, float* depth_out, int32_t* face_id_out,
                       int32_t* stats, void* stream);
int ossid_template_reduce(const uint8_t* color, const float* depth, int N, int T, int s, float* img_out, float* mask_out,
                          void* stream);

/* 8f-3d  texture-mapped meshes: BOP models whose .ply carries `comment TextureFile NAME` and per-vertex (u, v), the colour
 * living in the image. Build-defined, SPEC.md 7.15-7.17 (csrc/texture.hip, csrc/texture.h, csrc/raster.hip): the reference
 * renders such models with Blender / pyrender, neither in its tree.
 * ossid_texture_mips: image u8 [Ht][Wt][3] (RGB, row 0 the top row of the image file), 1 <= Ht, Wt <=
 * OSSID_TEXTURE_MAX_SIDE -> the mip chain in the caller's buffer `mips` (4-byte aligned, ossid_texture_mip_bytes(Ht, Wt)
 * bytes, 0 = bad sizes). Layout: 4 bytes per texel (R, G, B, 0); level 0 is the image, h_0 x w_0 = Ht x Wt; level l + 1
 * has h_{l+1} x w_{l+1} = ((h_l + 1) >> 1) x ((w_l + 1) >> 1) texels, down to 1 x 1 (ossid_texture_levels(Ht, Wt) levels,
 * 0 = bad sizes); level l starts at BYTE offset 4 * sum_{k<l} h_k w_k and is row-major. A texel of level l + 1 is, per
 * channel, (a + b + c + d + 2) / 4 (integer division) over rows 2y, 2y + 1 and columns 2x, 2x + 1 of level l, the odd ones
 * clamped to the last row / column: every level is made from the one before it. One launch per level.
 * ossid_raster_textured: ossid_raster_color with `colors` replaced by uvs f32 [V][2] = (u, v), v upwards, and the mip
 * chain of an Ht x Wt texture; the same workspace (ossid_raster_color_workspace_bytes) and the same first two launches, so
 * depth_out, face_id_out and stats are ossid_raster_color's bit for bit. The resolve interpolates (u, v)
 * perspective-correctly at the sample and at the samples of pixels (x + 1, y) and (x, y + 1), takes rho = the largest of
 * the four |differences| in level-0 texels, the level = the smallest l with rho <= 2^l (the top level when a neighbour's
 * denominator is <= 0 or a value is not finite), and fetches bilinearly with clamp-to-edge addressing at
 * s = u w_l - 0.5, t = (1 - v) h_l - 0.5. -> color_out u8 [N][H][W][3], lod_out int32 [N][H][W] (may be NULL; -1 where
 * nothing is drawn). UVs outside [0, 1] are legal; the caller refuses non-finite ones (the kernel then draws 0 and never
 * reads outside the chain). Three launches, nothing read back, capturable.
 * OSSID_EINVAL before any launch: what ossid_raster_color refuses, Ht or Wt outside [1, OSSID_TEXTURE_MAX_SIDE], a NULL
 * or misaligned mip buffer, mip_bytes below ossid_texture_mip_bytes(Ht, Wt). */
#define OSSID_TEXTURE_MAX_SIDE 8192
size_t ossid_texture_mip_bytes(int Ht, int Wt);
int ossid_texture_levels(int Ht, int Wt);
int ossid_texture_mips(const uint8_t* image, int Ht, int Wt, void* mips, size_t mip_bytes, void* stream);
int ossid_raster_textured(const float* vertices, int V, const int32_t* faces, int F, const float* uvs, const void* mips,
                          size_t mip_bytes, int Ht, int Wt, const float* transforms, int N, const float* intrinsics, int H, int W,
                          float pixel_offset, float z_near, void* workspace, size_t workspace_bytes, uint8_t* color_out,
                          float* depth_out, int32_t* face_id_out, int32_t* lod_out, int32_t* stats, void* stream);

/* 8f-4  the BOP-19 pose errors the reference's run ends with (scripts/online_learning.py:603-608:
 * saveResultsBop(..., run_eval_script=True); utils/bop_utils.py:51-53 shells out to bop_toolkit's scripts/eval_bop19.py
 * --renderer_type=cpp, which is not part of the reference tree). SPEC.md section 8 (csrc/bop_eval.hip): this build's own
 * restatement of the published definitions, parity with bop_toolkit unpinned. One length unit throughout, the caller's.
 * ossid_bop_vsd (8.3-8.5): depth_obs f32 [Fr][H][W] (a value that is not > 0 is invalid), cams f32 [Fr][4] = fx, fy, cx,
 * cy per frame, z_est and z_gt f32 [N][H][W] = ossid_raster_depth's renders (pixel_offset 0) of the estimates and of
 * their ground truths with the frame's camera, frame_host int32 [N] and taus_host f64 [T] in HOST memory (checked here,
 * passed on as kernel arguments) -> counts int32 [N][T+2] = (n_U, n_I, c_0 .. c_{T-1}), errors f64 [N][T]. A call may be a
 * chunk of a longer list. Integer counts by atomicAdd: bit-reproducible. Launches only, nothing read back, capturable --
 * with frame_host and taus_host read at call time: a captured graph replays with the frames and taus it was captured
 * with (the device buffers are read at replay as usual).
 * ossid_bop_mssd_mspd (8.7): vertices f32 [V][3], symmetries f64 [S][4][4] row-major (8.6), pose_est and pose_gt f64
 * [N][4][4], cams and frame_host as above -> mssd, mspd f64 [N] (mspd in pixels; +inf when a vertex is at Z <= 0 or not
 * finite under either pose for every symmetry).
 * OSSID_EINVAL before any launch: T outside [1, OSSID_BOP_MAX_TAUS], S outside [1, OSSID_BOP_MAX_SYMMETRIES], N < 1,
 * Fr < 1, a frame index outside [0, Fr), diameter not > 0, delta not >= 0, a non-finite tau, V outside
 * [1, OSSID_RASTER_MAX_VERTICES], H W outside (0, OSSID_RASTER_MAX_PIXELS], a NULL pointer. */
#define OSSID_BOP_MAX_TAUS 16
#define OSSID_BOP_MAX_SYMMETRIES 4096
int ossid_bop_vsd(const float* depth_obs, const float* cams, int Fr, int H, int W, const float* z_est, const float* z_gt,
                  const int32_t* frame_host, int N, double diameter, double delta, const double* taus_host, int T,
                  int32_t* counts, double* errors, void* stream);
int ossid_bop_mssd_mspd(const float* vertices, int V, const double* symmetries, int S, const double* pose_est,
                        const double* pose_gt, const float* cams, int Fr, const int32_t* frame_host, int N, double* mssd,
                        double* mspd, void* stream);
/* Several instances per target (SPEC.md 8.10-8.12; csrc/bop_eval.hip): BOP-19's errors between every kept estimate and
 * every ground-truth instance of a target, and its greedy matching per threshold. Caller-owned buffers, no workspace,
 * launches only, nothing read back, capturable. Still this build's restatement; parity with bop_toolkit unpinned.
 * ossid_bop_vsd_pairs (8.11): ossid_bop_vsd over a pair table. z_est f32 [Ne][H][W] and z_gt f32 [Ng][H][W] are two
 * separate stacks of ossid_raster_depth renders (each estimate and each instance rendered once); pairs int32 [P][3] =
 * (est_row, gt_row, frame) in DEVICE memory -> counts int32 [P][T+2], errors f64 [P][T], row p from the images the table
 * names, by ossid_bop_vsd's own per-pixel code. A row with est_row outside [0, Ne), gt_row outside [0, Ng) or frame
 * outside [0, Fr) is found on the device: no image is read, its counts are 0 and its errors 1.0; other rows are not
 * affected. taus_host as ossid_bop_vsd. OSSID_EINVAL before any launch: Ne, Ng, P or Fr < 1, and what ossid_bop_vsd
 * refuses of T, taus, diameter, delta, H W, NULL pointers.
 * ossid_bop_match (8.12): err f64 [Ptot][T+2] = per pair the T VSD errors, MSSD, MSPD; groups int32 [Gr][5] =
 * (pair_first, est_first, inst_first, E, G) per target: its E kept estimates in rank order are rows est_first .. of match,
 * its G instances entries inst_first .. of valid (u8, non-zero = counts towards tp), and its pairs, [e][g] row-major, rows
 * pair_first .. of err; thr f64 [Gr][T+2][10] the thresholds -> match int32 [Etot][T+2][10] = the instance (0 .. G-1) each
 * estimate is matched to per error kind and threshold column, -1 for none; tp int32 [T+2][10] = the matches whose
 * instance is valid, over all groups. Estimates in rank order; an estimate takes the not yet matched instance with
 * err < thr (strict, NaN never) of smallest error, the lowest index among equal errors. Both outputs are overwritten
 * (cleared by a kernel first). A group row with E outside [0, OSSID_BOP_MAX_INSTANCES], G outside [1,
 * OSSID_BOP_MAX_INSTANCES] or a range that leaves err, match or valid is skipped on the device: its estimates stay -1.
 * Integer atomics only: bit-reproducible. OSSID_EINVAL: Gr < 1, Itot < 1, Ptot or Etot < 0, T outside [1,
 * OSSID_BOP_MAX_TAUS], a NULL groups, valid, thr or tp, a NULL err with Ptot > 0 or match with Etot > 0. */
#define OSSID_BOP_MAX_INSTANCES 64
int ossid_bop_vsd_pairs(const float* depth_obs, const float* cams, int Fr, int H, int W, const float* z_est, int Ne,
                        const float* z_gt, int Ng, const int32_t* pairs, int P, double diameter, double delta,
                        const double* taus_host, int T, int32_t* counts, double* errors, void* stream);
int ossid_bop_match(const double* err, int Ptot, const int32_t* groups, int Gr, const uint8_t* valid, int Itot,
                    const double* thr, int T, int32_t* match, int Etot, int32_t* tp, void* stream);

/* Several instances per frame on the estimating side: distinct-pose selection (SPEC.md section 16;
 * csrc/pose_select.hip), this build's own definition -- the reference's loop keeps one pose per frame
 * (scripts/online_learning.py:466-469). Greedy non-maximum suppression over scored poses under 8.7's MSSD distance.
 * ossid_pose_select: poses f64 [N][4][4], scores f32 [N], points f32 [M][3], symmetries f64 [S][4][4] row-major (8.6; the
 * identity when the object has none), K picks, sep a length in the poses' unit, min_score (-inf for none) ->
 * selected int32 [K] (indices into poses in pick order, -1 past the last pick), count int32 [1] (the number of picks),
 * owner int32 [N] (the round whose pick suppressed the candidate, -1 = never owned). A candidate is eligible iff
 * scores[n] >= min_score (a NaN never is). Round r picks the eligible candidate without an owner of greatest score, the
 * lowest index among equal scores (+0 = -0), and gives it and every candidate without an owner at D(n, pick) <=
 * sep * sep the owner r, with D = min over symmetries of max over points of 8.7's squared distance q_v between the point
 * under poses[n] and under poses[pick] . S; no square root is taken. keys uint64 [K] is caller-owned scratch and an
 * output: keys[r] ends as round r's pick key (order-preserving score bits in the high word, the complemented index
 * 0xffffffff - pick in the low word), 0 for a round without a pick. All four are overwritten (cleared by a kernel first).
 * No workspace, 1 + 2 K launches whose grids depend on (N, M, S, K) alone, nothing read back, capturable. Integer
 * atomics, max and min only: bit-reproducible. OSSID_EINVAL before any launch, nothing written: N outside [1,
 * OSSID_SELECT_MAX_POSES], K outside [1, OSSID_BOP_MAX_INSTANCES], S outside [1, OSSID_BOP_MAX_SYMMETRIES], M outside
 * [1, 2^22], sep negative or not finite, a NaN min_score, a NULL pointer. */
#define OSSID_SELECT_MAX_POSES 65536
int ossid_pose_select(const double* poses, const float* scores, int N, const float* points, int M, const double* symmetries,
                      int S, int K, double sep, float min_score, int32_t* selected, int32_t* count, int32_t* owner,
                      uint64_t* keys, void* stream);

/* An object's symmetries from its own surface (SPEC.md section 17; csrc/symmetry.hip), this build's own definition --
 * BOP published its models_info.json symmetry lists without the procedure that made them, and the reference reads them.
 * Candidate rigid transforms are scored by how well they map a thinned sample of the surface (queries) onto a dense one
 * (targets); ossid_code_amd/symmetry.py generates the candidates and selects among them on the host.
 *
 * ossid_sym_grid: targets f32 [Nt][3] (finite; ossid_cloud_candidates' points are the intended input) -> the uniform
 * cell grid of 17.2 in `grid`, caller-owned, ossid_sym_grid_nbytes(Nt) bytes (0 = Nt outside [1, OSSID_SYM_MAX_TARGETS]),
 * 16-byte aligned, for acceptance at an f32 squared distance <= tol * tol. One workgroup; integer atomics place the points
 * and the order inside a cell does not reach any result.
 *
 * ossid_sym_score: the grid of ossid_sym_grid(targets, Nt, tol) (same Nt and tol), queries f32 [Mq][3], transforms f64
 * [C][4][4] row-major (rows 0-2 are read) -> per transform miss int32 [C] (queries without a target at d2 <= tol * tol; a
 * NaN query or transform misses), worst_d2 f32 [C] (the largest accepted d2, 0 when none), sum_q int64 [C] (the sum over
 * the accepted queries of trunc(f64(d2) / f64(tol * tol) * 2^32), 17.3). The point is transformed in f64 in 8.7's written
 * order, rounded to f32, and its nearest target is the lexicographic minimum of (d2, index). One workgroup per transform,
 * one launch, no atomics: bit-equal to the brute-force restatement. The grid's header records Nt and tol: a buffer whose
 * header does not carry this call's Nt and tol (bit for bit) and a consistent cell count is not followed, and every query
 * misses; the positions read from the cell table are clamped to the Nt sorted points, so no content of the buffer makes
 * the kernel read outside it.
 *
 * The size query ends in _nbytes, not in _grid_bytes like ossid_ppf_refine_grid_bytes: tests/test_workspace_contract.py
 * claims every symbol with that ending for the case table of tests/workspace_cases.py, and this buffer's contract (the
 * same run_contract) lives in tests/symmetry_cases.py and tests/test_symmetry_gpu.py instead.
 *
 * OSSID_EINVAL before any launch, nothing written: Nt outside [1, OSSID_SYM_MAX_TARGETS], Mq outside [1,
 * OSSID_SYM_MAX_QUERIES], C outside [1, OSSID_SYM_MAX_TRANSFORMS], a tol that is not finite and positive or whose f32
 * square is not, a NULL pointer, a grid buffer that is misaligned or shorter than ossid_sym_grid_nbytes(Nt). */
#define OSSID_SYM_MAX_TARGETS 32768
#define OSSID_SYM_MAX_QUERIES 4096
#define OSSID_SYM_MAX_TRANSFORMS 16384
size_t ossid_sym_grid_nbytes(int Nt);
int ossid_sym_grid(const float* targets, int Nt, float tol, void* grid, size_t grid_bytes, void* stream);
int ossid_sym_score(const void* grid, size_t grid_bytes, int Nt, const float* queries, int Mq, const double* transforms, int C,
                    float tol, int32_t* miss, float* worst_d2, int64_t* sum_q, void* stream);

/* 8f-6 the scorer's model cloud from the object's mesh (scripts/online_learning.py:303-311 loads model_points /
 * model_colors / model_normals from zephyr_model_data/{lmo,ycbv}/model_cloud_XX.npz, a download made by a script that is
 * in neither tree). SPEC.md section 9 (csrc/model_cloud.hip): this build's own definition, parity with zephyr's clouds
 * unpinned. Raw device pointers, caller-owned memory, launches only: nothing allocates, synchronises or is read back.
 * vertices f32 [V][3], faces int32 [F][3], colors u8 [V][3]; a face with an index outside [0, V) never votes and weighs 0.
 *
 * ossid_cloud_votes (9.2, online_learning.py:303-311): face_id int32 [n][H][W] (ossid_raster_color's face_id_out of n
 * views; a value outside [0, F) is no face), centres f64 [n][3] = the views' camera centres in the mesh's frame ->
 * votes int32 [F][2] += (samples that see the face from its front, t >= 0; from its back). The buffer ACCUMULATES: the
 * caller zeroes it before the first chunk of views. Integer atomicAdd after a run-length count per wave: bit-reproducible.
 *
 * ossid_cloud_weights (9.3, online_learning.py:303-311): votes -> weights u64 [F] (w_f, 0 = not usable), prefix u64 [F]
 * (inclusive sums in face order; prefix[F-1] = Wt, 0 = no usable face), normals f32 [F][3] (unit, turned to the side that
 * got more votes; 0 for a face that is not usable). Workspace: ossid_cloud_workspace_bytes(F) bytes (0 = bad F), 8-byte
 * aligned.
 *
 * ossid_cloud_candidates (9.4, online_learning.py:303-311): K stratified samples of the weighted faces -> points f32
 * [K][3], normals f32 [K][3], colors f32 [K][3] (in [0, 1]), face int32 [K] (-1 and zeros everywhere when Wt = 0). A face
 * that got more votes from its back is read as (p0, p2, p1): the cloud does not depend on how the mesh is wound.
 *
 * ossid_cloud_candidates_textured (9.4.1): the same candidates of a texture-mapped mesh -- points, normals and face are
 * ossid_cloud_candidates' bit for bit -- with colors_out = the bilinear fetch (7.17) at level lod in [0, top] of the mip
 * chain (ossid_texture_mips) at the affinely interpolated (u, v); uvs f32 [V][2]. OSSID_EINVAL also for Ht or Wt outside
 * [1, OSSID_TEXTURE_MAX_SIDE], a mip buffer that is NULL, misaligned or too small, lod outside [0, top].
 *
 * ossid_cloud_fps (9.5, online_learning.py:303-311): farthest-point sampling of M of K arbitrary FINITE f32 points
 * [K][3], from point 0, lowest index among equal maxima -> selection int32 [M] in pick order, radius f32 [M] (the
 * largest distance^2 to the earlier picks when pick j was chosen; radius[0] = +inf). One workgroup of 1024 threads.
 *
 * ossid_mesh_diameter (9.6, online_learning.py:303-311; what models_info.json calls `diameter`): out f64 [2] =
 * (D^2, D), D^2 the largest squared distance between two of the V <= OSSID_MESH_DIAMETER_MAX_VERTICES vertices.
 *
 * OSSID_EINVAL before any launch: a NULL pointer, V < 1, F outside [1, OSSID_RASTER_MAX_FACES], n < 1, H W outside
 * (0, OSSID_RASTER_MAX_PIXELS], M outside [1, OSSID_CLOUD_MAX_POINTS], K outside [M, OSSID_CLOUD_MAX_CANDIDATES] (fps)
 * or [1, OSSID_CLOUD_MAX_CANDIDATES] (candidates), a workspace that is too small. */
#define OSSID_CLOUD_MAX_POINTS 4096
#define OSSID_CLOUD_MAX_CANDIDATES 32768
#define OSSID_MESH_DIAMETER_MAX_VERTICES 262144
size_t ossid_cloud_workspace_bytes(int F);
int ossid_cloud_votes(const int32_t* face_id, int n, int H, int W, const float* vertices, int V, const int32_t* faces, int F,
                      const double* centres, int32_t* votes, void* stream);
int ossid_cloud_weights(const float* vertices, int V, const int32_t* faces, int F, const int32_t* votes, void* workspace,
                        size_t workspace_bytes, uint64_t* weights, uint64_t* prefix, float* normals, void* stream);
int ossid_cloud_candidates(const float* vertices, int V, const int32_t* faces, int F, const uint8_t* colors,
                           const int32_t* votes, const uint64_t* prefix, const float* normals, int K, float* points_out,
                           float* normals_out, float* colors_out, int32_t* face_out, void* stream);
int ossid_cloud_candidates_textured(const float* vertices, int V, const int32_t* faces, int F, const float* uvs, const void* mips,
                                    size_t mip_bytes, int Ht, int Wt, int lod, const int32_t* votes, const uint64_t* prefix,
                                    const float* normals, int K, float* points_out, float* normals_out, float* colors_out,
                                    int32_t* face_out, void* stream);
int ossid_cloud_fps(const float* points, int K, int M, int32_t* selection, float* radius, void* stream);
int ossid_mesh_diameter(const float* vertices, int V, double* out, void* stream);

/* 8f-7  detection mAP, the second figure the reference's run ends with (scripts/online_learning.py:615-618 ->
 * evalFinetuneResults, utils/detection.py:137-187, which shells out to an external script that is in neither tree). The
 * metric's arithmetic that IS in the reference tree: utils/detection_metrics.py:20-156,158-191 (DetectionMetric.calculate_mAP,
 * find_jaccard_overlap). SPEC.md section 10 (csrc/det_eval.hip): its sequential loop in an order-free form -- a detection is
 * a true positive iff it is the highest-ranked claimer of its ground truth. Raw device pointers, caller-owned memory,
 * launches only: nothing allocates, synchronises or is read back. A pointer may be NULL when its array is empty.
 *
 * ossid_det_claim (10.2-10.4): det_box f32 [N][4] = x1, y1, x2, y2 (16-byte aligned), det_score f32 [N], det_cls int32 [N]
 * in [0, C), det_image int32 [N] in [0, I), gt_box f32 [G][4] (16-byte aligned), gt_cls int32 [G], gt_offset int32 [I+1]
 * (CSR: image i owns the ground truths [gt_offset[i], gt_offset[i+1])) -> best_gt int32 [N] (-1 = none), best_iou f32 [N]
 * (0 then), sort_key int64 [N] = (cls << 32) | (0xFFFFFFFF - m(score)), m the order-preserving map of the float's bits
 * with -0 read as +0. The caller sorts the keys ascending and STABLY; the permutation is `order`, and class c owns the
 * ranks [class_offset[c], class_offset[c+1]) of it.
 *
 * ossid_det_match (10.5-10.8): order int32 [N], class_offset int32 [C+1], gt_difficult u8 [G] (NULL = none is),
 * iou_thr_host f32 [T] in HOST memory (read at call time, passed on as kernel arguments) -> status u8 [T][N] by INPUT
 * index (0 false positive: no match, 1 true positive, 2 ignored: its ground truth is difficult, 3 false positive:
 * duplicate), n_easy int32 [C], p11 f32 [T][C][11], ap11 f32 [T][C], apa f64 [T][C], map11 f32 [T], mapa f64 [T], and,
 * each unless NULL, the curves in RANK order: ctp, cfp int32 [T][N], prec, rec, env f32 [T][N]. Workspace:
 * ossid_det_eval_workspace_bytes(N, G, C, T) bytes (0 = a size outside its cap), 8-byte aligned. Integer atomicMin /
 * atomicMax / atomicAdd and fixed-order f64 sums only: bit-reproducible.
 *
 * OSSID_EINVAL before any launch: N outside [0, 2^22], G outside [0, 2^20], I outside [1, 2^20], C outside [1, 4096], T
 * outside [1, OSSID_DET_MAX_THRESHOLDS], a non-finite threshold, a NULL pointer to a non-empty array, a misaligned box
 * array or workspace, a workspace that is too small. The CONTENTS of the device arrays (finite numbers, indices inside their
 * ranges, ground truths grouped by image) are the caller's to check -- det_eval.py does; an index outside its range reads
 * nothing out of bounds here: such a detection has no candidate, such a rank is a false positive. */
#define OSSID_DET_MAX_THRESHOLDS 16
size_t ossid_det_eval_workspace_bytes(int N, int G, int C, int T);
int ossid_det_claim(const float* det_box, const float* det_score, const int32_t* det_cls, const int32_t* det_image, int N,
                    const float* gt_box, const int32_t* gt_cls, const int32_t* gt_offset, int G, int I, int C, int32_t* best_gt,
                    float* best_iou, int64_t* sort_key, void* stream);
int ossid_det_match(const int32_t* best_gt, const float* best_iou, const int32_t* order, const int32_t* class_offset, int N,
                    const int32_t* gt_cls, const uint8_t* gt_difficult, int G, int C, const float* iou_thr_host, int T,
                    void* workspace, size_t workspace_bytes, uint8_t* status, int32_t* n_easy, float* p11, float* ap11, double* apa,
                    float* map11, double* mapa, int32_t* ctp, int32_t* cfp, float* prec, float* rec, float* env, void* stream);

/* 8f-6  Keypoint-feature pose hypotheses (scripts/online_learning.py:52-76 getFeaturizedModels, :427 featurizeScene, :435
 * FeatureModel.match: zephyr's SIFT featurization in the reference), SPEC.md section 11. Raw device pointers, caller-owned
 * memory; counts that depend on the data stay on the device, so one frame is one launch chain with no host round trip.
 * Integer arithmetic, min / max and integer atomics only where results meet: bit-reproducible.
 *
 * ossid_feat_pyramid (11.1): img u8 [H][W][3] RGB -> pyramid, an int32 buffer of ossid_feat_pyramid_bytes(H, W, octaves)
 * bytes (0 = bad sizes: a side below 8, H W above OSSID_RASTER_MAX_PIXELS, octaves outside [1, OSSID_FEAT_MAX_OCTAVES]):
 * per octave o (side (side + 1) / 2 of the one before; an octave with a side below 8 and those after it do not exist) five
 * levels [5][Ho][Wo], octaves back to back, then two scratch planes.
 * ossid_feat_detect (11.2): depth f32 [H][W], mask u8 [H][W] -> keypoints int32 [max_keypoints][4] = (o, s, y, x) in
 * ascending order, count int32 [2] = the true number of keypoints, 1 iff it exceeds max_keypoints (then only the first
 * max_keypoints rows are written and every later stage treats the frame as having none). max_keypoints <=
 * OSSID_FEAT_MAX_KEYPOINTS. Workspace: ossid_feat_detect_workspace_bytes(H, W, octaves) bytes.
 * ossid_feat_describe (11.3-11.5), rows [0, count): bins int32 [max_keypoints] (orientation bin, -1 = window left the
 * image), descriptors u8 [max_keypoints][128] (values 0 .. 127), frames f64 [max_keypoints][4][4], ok u8 [max_keypoints]
 * (0 = dropped: its descriptor and frame rows are zero).
 * ossid_feat_match (11.7): the nearest of the Nm <= OSSID_FEAT_MAX_MODEL_FEATURES model descriptors u8 [Nm][128] for every
 * scene row with ok != 0 -> match int32 [max_keypoints][3] = (j, d2, w), (-1, 0, 0) for a skipped row or Nm = 0. Descriptor
 * arrays 16-byte aligned; workspace ossid_feat_match_workspace_bytes(max_keypoints) bytes, 8-byte aligned.
 * ossid_feat_hypotheses (11.8): T_i = F_s,i F_m,j^-1 -> cand_poses f64 [max_keypoints][4][4] and peaks int32
 * [max_keypoints][3] = (j, 0, w), the inputs of ossid_ppf_cluster(peaks, cand_poses, count, max_keypoints, 1, 1024, D, ...). */
#define OSSID_FEAT_MAX_KEYPOINTS 4096
#define OSSID_FEAT_MAX_MODEL_FEATURES 65536
#define OSSID_FEAT_MAX_OCTAVES 3
size_t ossid_feat_pyramid_bytes(int H, int W, int octaves);
int ossid_feat_pyramid(const uint8_t* img, int H, int W, int octaves, void* pyramid, size_t pyramid_bytes, void* stream);
size_t ossid_feat_detect_workspace_bytes(int H, int W, int octaves);
int ossid_feat_detect(const void* pyramid, int H, int W, int octaves, const float* depth, const uint8_t* mask, int contrast,
                      int max_keypoints, void* workspace, size_t workspace_bytes, int32_t* keypoints, int32_t* count,
                      void* stream);
int ossid_feat_describe(const void* pyramid, int H, int W, int octaves, const float* depth, float fx, float fy, float cx,
                        float cy, const int32_t* keypoints, const int32_t* count, int max_keypoints, int32_t* bins,
                        uint8_t* descriptors, double* frames, uint8_t* ok, void* stream);
size_t ossid_feat_match_workspace_bytes(int max_keypoints);
int ossid_feat_match(const uint8_t* scene_descriptors, const uint8_t* scene_ok, const int32_t* count, int max_keypoints,
                     const uint8_t* model_descriptors, int Nm, void* workspace, size_t workspace_bytes, int32_t* match,
                     void* stream);
int ossid_feat_hypotheses(const int32_t* match, const double* scene_frames, const int32_t* count, int max_keypoints,
                          const double* model_frames, int Nm, int32_t* peaks, double* cand_poses, void* stream);

/* 8f-8  cluttered multi-object RGB-D scenes of vertex-coloured and texture-mapped meshes with BOP ground truth, in place
 * of the offline BlenderProc renders the reference pre-trains on (datasets/render_dataset.py:81-189, datasets/dtoid_dataset.py:97-235) and of the depth corruption
 * it applies to them (utils/augmentation.py:5-26). SPEC.md section 13 (csrc/scene.hip): this build's own definition. Raw
 * device pointers, caller-owned memory, launches only: nothing allocates, synchronises or is read back; capturable.
 *
 * ossid_scene_desc -- a mesh atlas: vertices f32 [Vt][3], colors u8 [Vt][3], faces int32 [Ft][3] with indices LOCAL to
 * their mesh, meshes int32 [K][4] = (v0, nv, f0, nf); a draw list: instance_mesh int32 [I], transforms f32 [I][4][4]
 * row-major, scene_first int32 [S+1] (the instances of scene s are [scene_first[s], scene_first[s+1]); an empty scene is
 * legal), cams f32 [S][4] = fx, fy, cx, cy; and offsets int32 [I+1][2], the caller's prefix sums over the instances of
 * (ossid_scene_work_items(nf of the instance's mesh), nv of the instance's mesh), whose totals are work_items and records.
 * background u8 [Sb][H][W][3], Sb = 1 or S, may be NULL. Outputs: color_out u8 [S][H][W][3] (the background, or 0, where
 * nothing is drawn), depth_out f32 [S][H][W] (0 there), instance_out int32 [S][H][W] (the index into the draw list, -1
 * there), face_out int32 [S][H][W] (may be NULL; -1 there), facing_out f32 [S][H][W] (may be NULL; 0 there; SPEC 13.4),
 * amodal_out u32 [I][H][ceil(W / 32)]: bit x & 31 of word x >> 5 of row y is set iff a triangle of the instance covers the
 * sample of pixel (x, y), whatever hides it. pixel_offset and z_near as ossid_raster_depth.
 *
 * ossid_scene_render: one 64-bit key per (scene, pixel), bits(z) << 32 | instance - scene_first[s] << 22 | face, reduced by a
 * minimum: the nearest depth, among equal depths the lowest instance, then the lowest face. Per pixel the depth, colour
 * and face are those of ossid_raster_color's render of the winning instance alone, bit for bit. The workspace (16-byte
 * aligned, ossid_scene_workspace_bytes(records, S, H, W) bytes, 0 = bad sizes) holds the projected vertices and the keys.
 * Three launches. The CONTENTS of the device arrays are the caller's to check (scenes.py does); an instance whose table
 * entries lead outside an array is not drawn.
 *
 * ossid_scene_render_textured: ossid_scene_render for an atlas some of whose meshes are texture-mapped (SPEC 7.15-7.17,
 * 13.3): the same descriptor, workspace and three launches, and depth, instance, face, facing and the amodal masks are
 * ossid_scene_render's bit for bit. ossid_scene_tex adds uvs f32 [Vt][2] = (u, v), v upwards, beside the atlas's
 * vertices (the rows of a mesh without a texture are not read); mips, the meshes' mip chains (each in ossid_texture_mips'
 * layout) back to back, 4-byte aligned, mip_texels texels in all; tex_table int64 [K][3] = (first texel of the mesh's
 * chain in mips, Ht, Wt), Ht = 0 for a mesh drawn from its vertex colours (its other two entries are not read); and
 * lod_out int32 [S][H][W] (may be NULL). A pixel whose winning instance's mesh has Ht > 0 gets the colour and level
 * ossid_raster_textured gives that instance alone, from uvs + 2 v0 and the chain at mips + 4 t0 bytes; any other pixel is
 * coloured as by ossid_scene_render and has lod -1. desc->colors may hold anything in the rows of textured meshes. An
 * instance whose mesh's row has Ht < 0, Ht > 0 with Ht or Wt outside [1, OSSID_TEXTURE_MAX_SIDE], t0 < 0, or a chain that
 * ends past mip_texels is not drawn by any of the three launches: no texel outside [0, mip_texels) is addressed.
 *
 * ossid_scene_gt_info (13.5): amodal, instance_img = instance_out, sensor_depth f32 [S][H][W] -> gt_info int32 [I][12] =
 * (px_count_all, px_count_visib, px_count_valid, bbox_obj x y w h, bbox_visib x y w h, 0); an empty box is four -1s.
 * Integer atomics only: bit-reproducible. Three launches.
 *
 * ossid_scene_sensor (13.6): depth, facing f32 [S][H][W], thresholds f32 [S], n_rects int32 [S] (values are clamped to
 * [0, OSSID_SCENE_MAX_RECTS]), rects int32 [S][OSSID_SCENE_MAX_RECTS][4] = (r0, r1, c0, c1): a pixel keeps its depth iff
 * facing >= thresholds[s] and it lies in no rectangle (rows [r0, r1), columns [c0, c1)). q = rint((double) z * units) of a
 * kept pixel, 0 when that is not in [0, 65535] -> depth_u16 u16 [S][H][W] = q, depth_out f32 = (float)((double) q *
 * unit_inv), keep u8 (may be NULL). One launch; no random numbers.
 *
 * OSSID_EINVAL before any launch: a NULL pointer that is not optional, S outside [1, OSSID_SCENE_MAX_SCENES], I outside
 * [0, S * OSSID_SCENE_MAX_INSTANCES], H W outside (0, OSSID_RASTER_MAX_PIXELS], K < 1, Vt outside [1, 2^29], Ft outside
 * [0, 2^29], work_items outside [0, 2^30], records < 0, Sb not 1 or S with a background, pixel_offset outside [0, 1], z_near negative or not finite, units or unit_inv not positive and finite, a
 * workspace that is too small or misaligned; for ossid_scene_render_textured also a NULL tex_host, uvs, mips or tex_table,
 * a mips that is not 4-byte aligned, mip_texels < 1. */
#define OSSID_SCENE_MAX_SCENES 256
#define OSSID_SCENE_MAX_INSTANCES 1024
#define OSSID_SCENE_MAX_RECTS 6
typedef struct ossid_scene_desc {
    const float* vertices;
    const uint8_t* colors;
    const int32_t* faces;
    const int32_t* meshes;
    const int32_t* instance_mesh;
    const float* transforms;
    const int32_t* scene_first;
    const float* cams;
    const int32_t* offsets;
    const uint8_t* background;
    uint8_t* color_out;
    float* depth_out;
    int32_t* instance_out;
    int32_t* face_out;
    float* facing_out;
    uint32_t* amodal_out;
    int32_t Vt, Ft, K, I, S, H, W, Sb, work_items, records;
    float pixel_offset, z_near;
} ossid_scene_desc;
typedef struct ossid_scene_tex {
    const float* uvs;         /* f32 [Vt][2] = (u, v), v upwards; rows of meshes without a texture are not read */
    const void* mips;         /* the meshes' mip chains (ossid_texture_mips layout) back to back, 4-byte aligned */
    const int64_t* tex_table; /* int64 [K][3] = (first texel of the mesh's chain in `mips`, Ht, Wt); Ht = 0: vertex colours */
    int32_t* lod_out;         /* int32 [S][H][W], may be NULL: the level fetched; -1 where nothing is drawn or the winner is vertex-coloured */
    int64_t mip_texels;       /* texels in `mips` */
} ossid_scene_tex;
int ossid_scene_work_items(int n_faces);
size_t ossid_scene_workspace_bytes(int records, int S, int H, int W);
int ossid_scene_render(const ossid_scene_desc* desc_host, void* workspace, size_t workspace_bytes, void* stream);
int ossid_scene_render_textured(const ossid_scene_desc* desc_host, const ossid_scene_tex* tex_host, void* workspace,
                                size_t workspace_bytes, void* stream);
int ossid_scene_gt_info(const uint32_t* amodal, const int32_t* instance_img, const float* sensor_depth,
                        const int32_t* scene_first, int I, int S, int H, int W, int32_t* gt_info, void* stream);
int ossid_scene_sensor(const float* depth, const float* facing, int S, int H, int W, const float* thresholds,
                       const int32_t* n_rects, const int32_t* rects, double units, double unit_inv, uint16_t* depth_u16,
                       float* depth_out, uint8_t* keep, void* stream);

/* 8f-9  light for the scenes above (SPEC.md 13.10-13.11, csrc/scene_light.hip): this build's own definition, opt-in; the
 * render itself stays unlit. Raw device pointers, caller-owned memory, launches only; capturable. No new struct: the
 * pass takes the render's ossid_scene_desc.
 *
 * ossid_mesh_vertex_normals: smooth, area-weighted unit normals of ONE mesh, vertices f32 [V][3], faces int32 [F][3] ->
 * normals_out f32 [V][3]. Per face with all three indices in [0, V): n = (P1 - P0) x (P2 - P0) in f64 from the f32
 * coordinates; skipped when a component is not finite; q_c = llrint(ldexp(n_c, shift)) (half to even) is added to the
 * int64 accumulators of its three vertices by 64-bit integer atomics, so the sum does not depend on the order of
 * arrival. Per vertex s = (double) acc, nn = (sx sx + sy sy) + sz sz, the output (float)(s_c / sqrt(nn)), or (0, 0, 0)
 * unless nn > 0 (a vertex no face uses). shift is the caller's (scenes.normals_shift: the largest with
 * 2 e e 2^shift <= 2^40, e the largest extent of the finite vertices' bounding box; then no accumulator of at most
 * OSSID_RASTER_MAX_FACES terms reaches 2^63); with another shift a term outside int64 is the caller's error. Hard edges
 * are not detected: a mesh that wants them duplicates its vertices. The workspace holds the accumulators: int64 [V][3],
 * 8-byte aligned, ossid_mesh_vertex_normals_workspace_bytes(V) bytes (0 = V outside [1, 2^29]). Three launches: clear,
 * accumulate (none when F = 0), finish. OSSID_EINVAL before any launch, nothing written: a NULL vertices, normals_out or
 * workspace, NULL faces with F > 0, F outside [0, OSSID_RASTER_MAX_FACES], |shift| > 1000, a workspace that is too small
 * or misaligned.
 *
 * ossid_scene_light: a deferred shading pass over a rendered batch, one launch, one thread per (scene, pixel), no
 * workspace, no random numbers. Of desc_host it reads vertices, faces, meshes, instance_mesh, transforms, scene_first,
 * cams, Vt, Ft, K, I, S, H, W, pixel_offset, z_near (those of the render); colors, offsets, background and the output
 * pointers are not read and may be NULL. normals f32 [Vt][3] beside the atlas's vertices (each mesh's
 * ossid_mesh_vertex_normals); albedo u8 [S][H][W][3], instance and face int32 [S][H][W]: the render's color_out,
 * instance_out and face_out; lights f32 [S][OSSID_SCENE_MAX_LIGHTS][8] = (x, y, z, w, r, g, b, unused) in CAMERA space,
 * w == 0: (x, y, z) is the direction towards the light, otherwise the position of a point light; n_lights int32 [S]
 * (clamped to [0, OSSID_SCENE_MAX_LIGHTS]); ambient f32 [S][3]; material f32 [I][2] = (k_s, e), e truncated and clamped
 * to [0, 10] (not > 0, NaN included: 0): the Blinn-Phong exponent is 2^e. lit_out u8 [S][H][W][3] may be the SAME
 * buffer as albedo; normal_out f32 [S][H][W][3] (may be NULL): the unit shading normal in camera space, turned towards
 * the camera. Per pixel, SPEC 13.11: instance < 0 -> lit = albedo, normal 0. Otherwise the winner's three vertices are
 * projected again (7.2), its weights b0 b1 b2 and den are 7.12's, P = sum(b_j P_j) / den from the f32 camera points,
 * N = sum(b_j R n_j) from the f32-rotated vertex normals -- the face's own normal (13.4) when that sum has no finite
 * positive length --, lit_c = rint(albedo_c E_c + 255 (k_s Sp_c)) clamped to [0, 255] (NaN: 0) with E = ambient + sum_l
 * I_l max(0, N.L_l) and Sp = sum_l I_l (N.H_l)^(2^e) over the lights with N.L_l > 0, all in f64 in the written order. No
 * cast shadows, no attenuation, no light on the background; a non-uniform scale in transforms is not supported. With
 * ambient 1 and n_lights 0, lit == albedo. A pixel whose instance is not one of its scene's ([scene_first[s],
 * scene_first[s+1]) and < I), whose mesh entry leads outside [0, K), Vt or Ft, whose face is outside [0, nf) or has an
 * index outside [0, nv), an unusable vertex or zero area is copied through with normal 0: nothing outside an array is
 * addressed. OSSID_EINVAL before the launch: a NULL pointer other than normal_out (of the descriptor: vertices, meshes,
 * scene_first, cams; faces with Ft > 0; instance_mesh and transforms with I > 0), and the limits ossid_scene_render
 * applies to S, I, H W, K, Vt, Ft, pixel_offset and z_near. */
#define OSSID_SCENE_MAX_LIGHTS 4
size_t ossid_mesh_vertex_normals_workspace_bytes(int V);
int ossid_mesh_vertex_normals(const float* vertices, const int32_t* faces, int V, int F, int shift, void* workspace,
                              size_t workspace_bytes, float* normals_out, void* stream);
int ossid_scene_light(const ossid_scene_desc* desc_host, const float* normals, const uint8_t* albedo, const int32_t* instance,
                      const int32_t* face, const float* lights, const int32_t* n_lights, const float* ambient,
                      const float* material, uint8_t* lit_out, float* normal_out, void* stream);

/* 8f-10  cast shadows for the light above (SPEC.md 13.13-13.15, csrc/scene_shadow.hip and csrc/scene_light.hip): this
 * build's own definition, opt-in; ossid_scene_light is untouched. Raw device pointers, caller-owned memory, launches only;
 * capturable. No workspace and no size query: a triangle's vertices are projected by the thread that draws it.
 *
 * Shared arguments: light_views f32 [S][OSSID_SCENE_MAX_LIGHTS][16] = (R row-major 9, t 3, a, b, cx, cy), the light's view
 * of CAMERA space: Q = R P + t in f64 from the f32 rows in the written order ((r0 Px + r1 Py) + r2 Pz) + t; a point light
 * (lights[s][l][3] != 0) projects u = (Qx / Qz) a + cx, v = (Qy / Qz) b + cy, a directional one u = Qx a + cx, v = Qy b + cy.
 * scenes.shadow_views places them (13.15). shadow_map u32 [S][OSSID_SCENE_MAX_LIGHTS][Hs][Ws]: the bits of the nearest f32
 * light-space depth Qz per sample, 0x7f800000 where nothing is drawn; samples sit at pixel centres. z_near_l > 0.
 *
 * ossid_scene_shadow_maps: clears shadow_map and draws the draw list of desc_host (of which it reads what
 * ossid_scene_light reads, cams aside) into it, two launches (one when n = 0 or I = 0). items int32 [n][3] =
 * (s * OSSID_SCENE_MAX_LIGHTS + l, instance, first face): one wave per row draws the faces [first, first + 64) of the
 * instance's mesh from light l of scene s; the caller lists each (light, instance, 64 faces) it wants once
 * (scenes.shadow_views: every instance of the scene under every enabled light). Per face the three vertices' f32 camera
 * points (7.2) are projected as above; a vertex is usable iff Qz > z_near_l, Q, u and v are finite and |u|, |v| < 2^20, and
 * is snapped to rint(256 u), rint(256 v); a triangle with an unusable vertex or no area casts nothing (no clipping).
 * Coverage is 7.4-7.6's at samples 256 x + 128; the depth of a covered sample is perspective-correct for a point light
 * (7.7 on 1 / Qz) and ((w0 z0 + w1 z1) + w2 z2) / A in f64 for a directional one, rounded to f32, reduced by a 32-bit
 * unsigned minimum on its bits: bit-reproducible. A row whose first entry is outside [0, 4 S), whose instance is not one
 * of scene s, whose mesh entry leads outside [0, K), Vt or Ft or whose first face is outside [0, nf) is skipped, as is a
 * face with an index outside [0, nv): nothing outside an array is addressed. lights is read for the w column alone.
 * OSSID_EINVAL before any launch: a NULL pointer (items with n = 0 aside), n outside [0, 2^30], Hs or Ws outside [1, 4096],
 * z_near_l not positive and finite, and what ossid_scene_light refuses of desc_host.
 *
 * ossid_scene_light_shadowed: ossid_scene_light -- the same arguments, the same steps 1-8 of SPEC 13.11, stated once in
 * the source -- with each light's diffuse and specular term scaled by its visibility at the pixel's surface point P
 * (13.14): enable int32 [S][OSSID_SCENE_MAX_LIGHTS] (0: the light casts no shadow), shadow_params f32 [S][2] = (beta0,
 * beta1). For a light with N.L > 0 and enable != 0: Q, u, v of P as above; vis = 1 unless Qz > z_near_l and Q, u, v are
 * finite; texel = Qz / a (point) or 1 / a (directional), tan = sqrt(max(1 - (N.L)^2, 0)) / N.L, bias = texel (beta0 +
 * beta1 min(tan, 8)); k counts the taps (floor(u) + dx, floor(v) + dy), dx, dy in {-1, 0, 1}, that lie inside the map, are
 * not 0x7f800000 and hold a depth < Qz - bias (compared in f64); vis = (double)(9 - k) / 9.0; the terms are I (N.L vis) and
 * I ((N.H)^(2^e) vis). Ambient light is not shadowed. blocked_out u8 [S][H][W] (may be NULL): the sum of k over the
 * pixel's lights, at most 36; 0 on the background and on a pixel that is copied through. With enable all 0, lit_out and
 * normal_out are ossid_scene_light's byte for byte. No cube maps (a point light shadows inside its one frustum), no
 * clipping at the light's near plane, no shadow on the background. One launch. OSSID_EINVAL before it: what
 * ossid_scene_light refuses, a NULL shadow_map, light_views, enable or shadow_params, Hs or Ws outside [1, 4096], z_near_l
 * not positive and finite. */
int ossid_scene_shadow_maps(const ossid_scene_desc* desc_host, const float* lights, const float* light_views,
                            const int32_t* items, int n, int Hs, int Ws, float z_near_l, uint32_t* shadow_map, void* stream);
int ossid_scene_light_shadowed(const ossid_scene_desc* desc_host, const float* normals, const uint8_t* albedo,
                               const int32_t* instance, const int32_t* face, const float* lights, const int32_t* n_lights,
                               const float* ambient, const float* material, const uint32_t* shadow_map, const float* light_views,
                               const int32_t* enable, int Hs, int Ws, float z_near_l, const float* shadow_params,
                               uint8_t* lit_out, float* normal_out, uint8_t* blocked_out, void* stream);

/* 8f-11  objects at rest on a table (SPEC.md 13.16-13.18, csrc/scene_rest.hip): this build's own definition, opt-in, in
 * place of the physics engine BlenderProc drops the reference's objects with (datasets/render_dataset.py:81-189). Raw
 * device pointers, caller-owned memory, one launch each, no workspace, nothing read back, no random numbers, no float
 * atomics; capturable (ossid_scene_drop with G > 110 after one call outside a capture, which raises the kernel's LDS
 * limit). Every result is a maximum: order-independent and bit-reproducible. No struct and no changed signature: the ABI
 * version stays, as for 8f-8 to 8f-10.
 *
 * ossid_mesh_support (13.16): vertices f32 [V][3], dirs f64 [D][3] -> h_out f64 [D], h[d] the maximum over the vertices
 * whose three coordinates are finite of ((dx x + dy y) + dz z) in f64 from the (double) f32 coordinates, written order, no
 * contraction; a term that is NaN (a direction that is not finite) never replaces the running maximum; -inf when no
 * vertex is finite. +0 and -0 compare equal: which of them is returned is not defined. One workgroup takes 8 directions
 * and walks every vertex. OSSID_EINVAL before the launch: a NULL pointer, V outside [1, OSSID_RASTER_MAX_VERTICES], D
 * outside [1, OSSID_REST_MAX_DIRS].
 *
 * ossid_scene_drop (13.18): vertices, faces, meshes [K][4], Vt, Ft, K: the atlas as ossid_scene_desc names it;
 * instance_mesh int32 [I], scene_first int32 [S+1]; local f64 [I][12], a 3x4 row-major map from model to TABLE frame (z'
 * up, the table at z' = 0): p_c = ((L_c0 x + L_c1 y) + L_c2 z) + L_c3 in f64. One workgroup per scene holds a height
 * field H f32 [G][G] in LDS, cell (iy, ix) = [x0 + ix cell, x0 + (ix + 1) cell) x [x0 + iy cell, ...), x0 = -(G / 2)
 * cell (G / 2 = 0.5 G, not truncated), all +0 at first, and places the scene's instances one after another in draw order. A triangle is
 * usable iff its three indices lie in [0, nv) and its nine transformed coordinates are finite; its cells are those of its
 * bounding box, ix in [floor((xmin - x0) / cell), floor((xmax - x0) / cell)] within [0, G - 1], likewise iy. Pass 1:
 * zlow = min of zmin, off = max(-zlow, max over usable triangles and their in-grid cells of ((double) H[cell] - zmin)).
 * Pass 2: H[cell] = v where v > H[cell], v = zmax + off rounded UP to f32 (v >= 0: an integer maximum on its bits).
 * drop[i] = off, status[i] = 0, or 2 when a usable triangle has a cell of its box outside the grid (the table term -zlow
 * holds for it all the same). An instance without a usable triangle -- or whose instance_mesh or table row leads outside
 * [0, K), Vt or Ft -- gets status 1, drop 0 and leaves H as it was. A scene whose scene_first entries are not 0 <= first
 * <= last <= I places nothing. height_out f32 [S][G][G] (may be NULL): the final fields. Nothing outside an array is
 * addressed. OSSID_EINVAL before the launch: S outside [1, OSSID_SCENE_MAX_SCENES], I outside [0, S *
 * OSSID_SCENE_MAX_INSTANCES], K < 1, Vt outside [1, 2^29], Ft outside [0, 2^29], G outside [1, OSSID_REST_MAX_GRID], cell
 * not finite or not > 0, a NULL vertices, meshes or scene_first, NULL faces with Ft > 0, a NULL instance_mesh, local,
 * drop or status with I > 0. */
#define OSSID_REST_MAX_DIRS 16384
#define OSSID_REST_MAX_GRID 128
int ossid_mesh_support(const float* vertices, int V, const double* dirs, int D, double* h_out, void* stream);
int ossid_scene_drop(const float* vertices, const int32_t* faces, const int32_t* meshes, int Vt, int Ft, int K,
                     const int32_t* instance_mesh, const int32_t* scene_first, const double* local, int I, int S, int G,
                     double cell, double* drop, int32_t* status, float* height_out, void* stream);

/* =============================================================================================
 * Detector pre-training on rendered scenes (SPEC.md section 15; python/ossid/train.py over
 * datasets/dtoid_dataset.py:97-236 in the reference, which reads offline BlenderProc renders)
 * ============================================================================================= */

/* ossid_scene_dtoid_batch: T chosen targets of a rendered scene batch -> the detector's training batch, one launch, no
 * random numbers. color u8 [S][H][W][3], instance int32 [S][H][W] and gt_info int32 [I][12] are ossid_scene_render's and
 * ossid_scene_gt_info's outputs; targets int32 [T][2] = (scene s, instance i); jitter f32 [T][8] =
 * (g_r, g_g, g_b, b_r, b_g, b_b, a, seed -- read as its 32 bits) or NULL (15.3).
 *   img_out     f32 [T][3][H][W]   (float)u8 / 255.0f, the bits of ossid_dtoid_prep_sample's equal-size path; with a
 *                                  jitter row, 15.3's steps on top, clamped to [0, 1]
 *   mask_out    f32 [T][1][H][W]   1 where instance[s] == i, else 0
 *   bbox_out    f32 [T][1][5]      (x, y, x+w-1, y+h-1, 1) from gt_info's bbox_visib; (2^30, 2^30, -1, -1, -1) when empty
 *   heatmap_out f64 [T][1][heat_h][heat_w]   ossid_mask_bbox_heatmap's formula around that box's centre with
 *                                  scale = (double)heat_h / (double)H and `sigma`; zeros for an empty box
 * A target row with s outside [0, S) or i outside [0, I) writes zeros everywhere and the empty box and reads nothing of
 * the inputs. Refused before a launch: a NULL buffer (jitter aside), a size or sigma that is not positive, T < 1,
 * H*W >= 2^30, heat_h*heat_w >= 2^30. */
int ossid_scene_dtoid_batch(const uint8_t* color, const int32_t* instance, const int32_t* gt_info, int S, int H, int W,
                            int I, const int32_t* targets, int T, const float* jitter, int heat_h, int heat_w, double sigma,
                            float* img_out, float* mask_out, float* bbox_out, double* heatmap_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSSID_HIP_H */
