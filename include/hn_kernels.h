/*
 * hn_kernels.h — C ABI of the MI355X (gfx950) HyperNeRF render hot path.
 *
 * The reference (songrise/HyperNeRF-torch) has no FFI/plugin boundary: its hot path is plain
 * PyTorch behind Python call signatures.  This header is the boundary a native
 * replacement needs: plain pointers + sizes, caller-allocated buffers, launch on the caller's
 * stream, int status (0 = ok, <0 = argument error, >0 = hipError_t).  No allocation, no host
 * synchronisation, no global mutable state inside — every entry point is re-entrant and
 * graph-capturable.  Random draws (t_rand, u, noise) are explicit input buffers.
 *
 * Each entry point cites the reference code it replaces (paths relative to the reference repo).
 *
 * The dense part of the path (modules.MLP and everything built from it) runs on a small
 * "MLP machine": per 32-point block a wavefront keeps the hidden activation in registers with
 * points on the lane axis and features on the register axis, so an MFMA accumulator tile is the
 * next layer's B operand without touching LDS; weights are pre-packed into MFMA A-fragment order
 * (hn_pack_units) and streamed through LDS by LDS-DMA.  The host describes a network as a short
 * program of ops (HN_OP_* / HN_BOP_*), so every constructor configuration of the reference's
 * modules maps onto the same three kernels (forward, backward-data, weight-gradient).
 */
#ifndef HN_KERNELS_H
#define HN_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hnStream_t; /* hipStream_t */

#define HN_VERSION 340   /* 320: HnDwJob carries a second X slot; 321: HN_BOP_AUX w2 = tile word; 330: a level composited
                            from two parts through a merge permutation (HnCompositeArgs.perm, hn_sample_pdf_split); 331: weight-gradient
                            jobs flush to partial slabs + hn_mlp_wgrad_reduce (HnDwBatch.partials, HnDwJob.p_tile); 340: hn_build_config,
                            hn_mlp_wgrad_reduce_adam (the reduce launch applies the optimizer).  The activations
                            HN_ACT_LEAKY_RELU / ELU / SOFTPLUS extend the op-word vocabulary only: no struct and
                            no existing encoding changed */

/* numeric modes of the MLP machine */
#define HN_MODE_F32 0  /* v_mfma_f32_32x32x2_f32: exact fp32 products, parity mode (<=1e-4 vs oracle) */
#define HN_MODE_BF16 1 /* v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulate, throughput mode   */
/* OPT-IN, not the mode the bench line is quoted on: HN_MODE_BF16 in every product of the forward and backward-data
 * machines and in every output, but the training stash (layer inputs X, layer gradients dZ — what ONLY the weight
 * gradient reads) is kept in 8 bits: X as OCP e4m3, dZ as OCP e5m2 of 2^dz_scale_log2 * dZ, 1 KiB per 32x32 tile
 * instead of 2; the weight-gradient kernel multiplies them with v_mfma_f32_32x32x16_bf8_fp8 (fp32 accumulate) and
 * undoes the scale.  Halves the stash traffic that bounds a training step; costs rounding noise in dW only
 * (DESIGN.md section 8).  hn_mlp_wgrad* take the scale in their mode argument: HN_MODE_BF16_S8 | dz_scale_log2 << 8. */
#define HN_MODE_BF16_S8 2

#define HN_MAX_SRC 8 /* forward: feature sources 0-3 ; backward: 0-3 same, 4-7 gradient inputs */
#define HN_MAX_DST 4
#define HN_MAX_SLOTS 128
#define HN_OP_WORDS 8
#ifndef HN_CHUNK_UNITS
#define HN_CHUNK_UNITS 32 /* weight stream is consumed in chunks of 32 units of 1 KiB */
#endif
#define HN_DSRC_COMPS 32  /* per-point source-gradient accumulators in the backward machine */

/* ---- forward ops: word0 = opcode ---------------------------------------------------------
 * Machine state per wavefront (32 points): `cur` = current hidden activation (<= 256 features) as
 * MFMA B fragments, `accL` = the last accumulator tile (pre-activation) for the OUT ops.
 *
 * HN_OP_LAYER: one Linear (+bias, +activation).  Input features = [cur (32*K32) | nG groups of 64
 * GENERATED features (feature table)].  For every 32-row output tile t < NT, one at a time:
 *     acc = bias[32t..] + W[32t.., main] . cur + W[32t.., aux] . generated ;  nxt[t] = act(acc)
 * then cur <- nxt (unless NO_COMMIT).  Weight-stream order per tile: K32 main blocks, then 2*nG
 * aux blocks (a "block" = 32 out x 32 in).  Training: relu bit mask -> mask_slot, activation ->
 * stash_out (X of the next layer's dW), generated features -> stash_aux.  The stash is a workspace of the three
 * machine kernels, opaque to the host: bf16 mode stores the operand fragments as they are (the weight-gradient kernel
 * transposes on its LDS read), fp32 mode stores tiles transposed through the matrix core. */
#define HN_OP_LAYER 1    /* w1 = K32 | nG<<8 | NT<<16 | act<<24 | flags<<28 ; w2=bias_off w3=feat_off
                            w4=mask|-1 w5=stash_out|-1 w6=stash_aux|-1 — RESOLVED for the launch: the byte offset
                            of block 0 of that stash region in KiB (masks: in units of 256 B); a region holds, per
                            32-point block, NT tiles (out), 2*nG tiles (aux) or (NT+1)/2 mask words per lane;
                            w7 = first activation parameter p0 (bit-cast float, 0 for NONE / RELU).
                            HN_ACT_SOFTPLUS keeps no mask: its w4 is the second parameter p1 (bit-cast float)     */
/* act(z), z = the fp32 accumulator (pre-activation).  The backward takes f' from what it has: the mask word (RELU,
 * LEAKY_RELU) or the layer output y read back from the stash slot the forward wrote (ELU, SOFTPLUS).  Activations whose
 * derivative is not a function of y (SiLU, GELU) would need the pre-activation stashed and are not provided. */
#define HN_ACT_NONE 0
#define HN_ACT_RELU 1
#define HN_ACT_LEAKY_RELU 2 /* z > 0 ? z : p0*z (p0 = negative_slope); mask word as RELU; f' = keep ? 1 : p0           */
#define HN_ACT_ELU 3        /* z > 0 ? z : p0*expm1(z) (p0 = alpha); f' = y > 0 ? 1 : y + p0                           */
#define HN_ACT_SOFTPLUS 4   /* p0*z > p1 ? z : log1p(exp(p0*z))/p0 (p0 = beta, p1 = threshold); f' = p0*y > p1 ? 1 :
                               1 - exp(-p0*y)                                                                           */
#define HN_LAYER_NO_COMMIT 1 /* flags bit0: leave cur untouched (head layers read by an OUT op)      */
#define HN_LAYER_DIRECT 2    /* flags bit1: the layer's feature groups hold HN_FEAT_ID_DIRECT entries       */
/* dst[w1][p*ld + w2 + i] = act(accL row i) (+ residual src[w5][.. + w6 + i]), i < w3 <= 4           */
#define HN_OP_OUT 4      /* w1=dst  w2=col  w3=n  w4=act(0 none,1 sigmoid)  w5=res_src|-1  w6=res_col
                            w7 = 1 + first staged component the n results are ALSO published to (0 = none): later
                            layers of the same program encode them as generated features (warp -> template) */
#define HN_OP_OUT_WIDE 5 /* w1=dst  w2=col  w3=n (<= 32*NT)  w4=NT   (cur features -> dst)            */

/* ---- backward ops ---------------------------------------------------------------------------
 * State: `cur` = dZ of the layer being differentiated, `cur2` = a second, 32-feature dZ (heads).
 * HN_BOP_LAYER: dH = W^T . dZ for every 32-feature tile t < NT of the layer INPUT, one at a time:
 *     acc = W[:, 32t..]^T . cur (32*K32 dZ features) + W2[:, 32t..]^T . cur2 (if K32b) ;
 *     nxt[t] = acc * f'(mask | y) ; then cur <- nxt.  Stream order per tile: K32 blocks, K32b blocks. */
#define HN_BOP_LOAD 1      /* w1=src w2=col w3=n(<=4) w4=act'(1 sigmoid: y from src w5 col w6)
                              w7=stash|-1 ; w3 bit 8 set: destination cur2 instead of cur ;
                              w3 bit 9 set: ADD the source-gradient accumulators of slots 8*((w3>>10)&3) + i — the
                              gradient that later ops of this program (earlier in forward order) left for the
                              components this head published (a NULL src then contributes nothing)         */
#define HN_BOP_LOAD_WIDE 2 /* w1=src  w2=col  w3=n | dact<<16  w4=NT  w5=relu mask|-1  w6=p0  w7=dZ stash|-1
                              (resolved offsets).  dact = HN_ACT_* of the output when f' is more than the mask AND
                              (LEAKY_RELU, ELU, SOFTPLUS), else 0.  ELU / SOFTPLUS: the derivative source is the dZ
                              slot itself — the forward layer stashed y there (its stash_out) and this op overwrites
                              it, tile by tile and lane by lane, with dZ; SOFTPLUS has no mask, w5 = p1              */
#define HN_BOP_LAYER 3     /* w1 = K32 | K32b<<8 | NT<<16 ; w4=mask|-1 w5=dZ stash|-1 (resolved offsets) ;
                              w2 = dact of the layer's activation (as HN_BOP_LOAD_WIDE; 0 = the mask AND / none),
                              w3 = p0, w7 = p1 (bit-cast floats), w6 = derivative source: the stash slot of the layer
                              output y (its stash_out, resolved offset; ELU / SOFTPLUS, else unused)                 */
/* gradient w.r.t. GENERATED input features: per 32-feature tile of nG*64 features,
 * tmp = W_aux^T . (cur | cur2), then the chain rule through the feature table into the per-point
 * source-gradient accumulators (LDS), written to `dsrc` at the end of the program.               */
#define HN_BOP_AUX 4       /* w1 = K32 | K32b<<8 | nG<<16 ; w3=feat_off ; w2 = tile word: bit tt = tile tt (of 2*nG) holds
                              a feature with a gradient — only those tiles are in the weight stream and computed —,
                              bit 8+tt = one of them is trigonometric (else d feature / dx = 1, no factor applied)  */

/* feature table entry (8 bytes).  value(p) = kind(freq * x), x = staged source component `ci` of point p.
 * The distinct (source, column) pairs a program reads are listed once in HnMlpArgs.comps; every workgroup
 * stages them per 32-point block into LDS, so evaluating a feature costs two LDS reads and no global load. */
typedef struct {
  int32_t packed; /* bits 0-7 ci (index into comps) | 12-15 kind | 16-23 grad slot + 1 (0 = no gradient) */
  float freq;
} HnFeat;
#define HN_MAX_COMPS 32 /* staged source components per program */
#define HN_FEAT_ID_DIRECT 5 /* identity feature read straight from global memory: src in bits 8-11, column in
                               bits 24-31 (stand-alone modules with > HN_MAX_COMPS raw input channels) */
#define HN_FEAT_ZERO 0
#define HN_FEAT_ID 1
#define HN_FEAT_SIN 2  /* sin(freq*x)                                                        */
#define HN_FEAT_COS 3  /* cos(freq*x)                                                        */
#define HN_FEAT_SINP 4 /* sin(freq*x + 0.5*3.1415926): the reference's cosine in model_utils.posenc:262 */

typedef struct {
  const float* ptr; /* NULL: the source is absent — its staged components are left to the program itself (HN_OP_OUT
                       publishes head outputs as components, fused level programs) / its gradient input is zero */
  int32_t ld;      /* row stride in floats */
  int32_t per_ray; /* 1: row index = point / samples_per_ray, 0: row index = point */
  const int64_t* gather_idx; /* optional (per_ray sources): row index = gather_idx[ray] — the GLO embedding lookup
                                (modules.GLOEmbed, hypernerf/modules.py:155-167) read straight from the table;
                                an index outside [0, gather_rows) stages NaN */
  int32_t gather_rows;
  int32_t pad;
} HnSrc;

typedef struct {
  float* ptr;
  int32_t ld;
  int32_t pad;
} HnDst;

typedef struct {
  uint64_t off; /* byte offset from the stash / mask base for block 0 */
  int32_t nt;   /* stash: 32-feature tiles per block ; mask: dwords per lane per block */
  int32_t pad;
} HnSlot;

/* One launch of the forward or backward machine over n_points points.
 * Replaces, per launch: modules.MLP.forward (hypernerf/modules.py:116-127) and the modules
 * composed from it — TranslationField.warp (hypernerf/warping.py:90-96), HyperSheetMLP.forward
 * (hypernerf/modules.py:331-337), NerfMLP.forward (hypernerf/modules.py:266-298), the encoders
 * model_utils.posenc_orig / posenc (hypernerf/model_utils.py:234-274) fused as generated input
 * features, legacy models/nerf.py:83-124 — and, for the backward machine, their autograd. */
typedef struct {
  int32_t mode;            /* HN_MODE_* */
  int32_t n_points;        /* P */
  int32_t samples_per_ray; /* S (ray(p) = p / S) */
  int32_t training;        /* 0: skip mask/stash writes */
  int32_t n_ops;
  int32_t n_chunks; /* weight stream length in chunks of HN_CHUNK_UNITS KiB */
  int32_t n_dsrc;   /* backward: number of source-gradient components written per point (<=16) */
  int32_t n_bias;   /* floats in `bias` (staged into LDS once per workgroup) */
  int32_t n_feat;   /* entries in `feat` (staged into LDS once per workgroup) */
  int32_t max_groups; /* most feature groups any one layer has (the forward machine is built for <=2 and for 3) */
  const int32_t* ops;    /* device, n_ops * HN_OP_WORDS */
  const void* wstream;   /* device, packed weight units (hn_pack_units) */
  const float* bias;     /* device, packed biases (fp32) */
  const HnFeat* feat;    /* device, feature table */
  void* stash;           /* device, activation / dZ stash (training) */
  uint32_t* masks;       /* device, relu bit masks (training) */
  float* dsrc;           /* backward: [P][n_dsrc] source gradients */
  HnSrc src[HN_MAX_SRC]; /* forward: feature sources ; backward: same + gradient inputs */
  HnDst dst[HN_MAX_DST];
  HnSlot slots[HN_MAX_SLOTS]; /* unused by the kernels since ABI 200 (the op words carry resolved offsets); kept for
                                 hosts that want to hand the layout along */
  uint64_t* prof;        /* diagnostic only (NULL in production): 8 shader-clock sums, see tools/ */
  const int32_t* comps;  /* device, n_comps entries: src << 16 | column */
  int32_t n_comps;
  int32_t embed_reg_mask; /* backward, 0 = off: bit i set = accumulator register i holds (in one lane half or both)
                             a source-gradient slot of the gathered per-ray source; those are summed over the 32
                             points of the block (all of ONE ray: samples_per_ray % 32 == 0 is required) and added to
                             embed_grad[gather_idx[ray]][embed_col[slot]] — GLOEmbed's backward, scatter included */
  float* embed_grad;      /* (gather_rows, embed_dim) fp32, accumulated with float atomics */
  const int64_t* embed_idx;
  int32_t embed_rows, embed_dim;
  int8_t embed_col[HN_DSRC_COMPS]; /* slot -> column of the table row, -1 = not an embedding component */
  int32_t n_trig_comps;   /* forward, bf16: staged components 0 .. n_trig_comps-1 also get x / 2pi staged as hi + lo
                             (every component a trigonometric feature reads must be among them; >= 1 if n_comps > 0) */
  int32_t wide_ops;       /* bit 0: the op program holds HN_OP_OUT_WIDE / HN_BOP_LOAD_WIDE ops; bit 1: its feature table
                             holds HN_FEAT_ID_DIRECT entries (layers flagged HN_LAYER_DIRECT).  Forward launches take
                             the kernel build that carries those paths if either bit is set, backward launches if bit 0
                             is; 0 selects the builds without them (what every render-level program runs: no scratch).
                             bit 2: every layer of the program is ReLU or linear (no LeakyReLU / ELU / Softplus op words).
                             With bit 2 set, bits 0 and 1 clear and mode HN_MODE_BF16 the launches take the lean ReLU-only
                             builds (hn_mlp_fwd_relu_kernel / hn_mlp_bwd_relu_kernel: same results bit for bit, less code);
                             a caller that leaves the bit clear gets the generic builds, which run every program */
  int32_t dz_scale_log2;  /* HN_MODE_BF16_S8, backward: the machine carries 2^dz_scale_log2 * dZ (exact: a power of two)
                             so that the e5m2 stash keeps small gradients; source / embedding gradients leave unscaled */
  int32_t trig_lo_planes; /* 1: the lo planes are staged (exactly reduced sine arguments); 0: hi only + one shared zero
                             plane (programs whose staging would not fit into LDS otherwise: hn_mlp_forward returns -6
                             when ring + tables + 8 waves x (n_comps + n_trig + (lo ? n_trig : 1)) x 128 B > 158 KiB) */
  uint64_t* timeline;     /* optional (ABI 330), device uint64[8], zero-initialised by the caller once: the launch times
                             itself — [4] += last workgroup's end - first workgroup's start in ticks of the 100 MHz
                             wall clock, [5] += 1, [0]/[1] start / end of the last run, [6]/[7] first start / last end
                             ever; [2], [3] are tickets the launch leaves at zero.  Lets a step that is replayed as one
                             HIP graph report per-kernel durations of the timed replays themselves.  NULL = off. */
  float* embed_partial;   /* backward, optional (ABI 331): with embed_reg_mask set, the per-block sums of the gathered
                             row's gradient are STORED to embed_partial[block][embed_dim] (columns without a gradient
                             slot are left untouched) instead of added to embed_grad by float atomics;
                             hn_mlp_wgrad_reduce (HnEmbedReduce) then sums them per table row in a fixed order */
} HnMlpArgs;

/* weight packing: one descriptor per 1-KiB unit of a stream */
typedef struct {
  int32_t w_id;       /* index into the pointer table ; -1 = all-zero unit */
  int32_t ld;         /* source row stride (in_features) */
  int32_t r0, c0;     /* source row / col of A-operand (row 0, k 0) */
  int32_t r_end;      /* valid source rows  [.., r_end)  */
  int32_t c_end;      /* valid source cols  [.., c_end)  */
  int32_t k0;         /* first k feature of this unit within the 32-block (bf16: 0/16 ; f32: 4*g steps) */
  int32_t transposed; /* 0: A[row][k] = W[r0+row][c0+k] ; 1: A[row][k] = W[r0+k][c0+row] */
} HnPackUnit;

typedef struct {
  int32_t w_id; /* bias vector id or -1 */
  int32_t n;    /* valid length */
  int32_t off;  /* destination offset (floats) */
  int32_t len;  /* padded length */
} HnPackBias;

/* weight-gradient job: one workgroup (8 waves) accumulates the dW tile grid n_nt x n_kt of one Linear input
 * segment over a block range; pad = gn | gk<<8 | bps<<16: gn x gk (<= 8 waves) is the wave grid, each wave
 * owns a ceil(n_nt/gn) x ceil(n_kt/gk) (<= 4x2) tile rectangle; bps = point blocks per LDS stage
 * (bps * (n_nt+n_kt) tiles <= 32 KiB).  n_nt, n_kt <= 8 tiles (bf16) / 4 tiles (fp32).
 * The k-tiles may come from TWO stash slots (a skip layer's running activation followed by its re-appended encoder
 * input, hypernerf/modules.py:122-124): tiles 0 .. n_kt1-1 from (x_off, x_nt, x_t0), the rest from (x2_off, x2_nt,
 * x2_t0) — one job, one read of the dZ tiles, instead of one job per segment.  n_kt1 == n_kt: one slot. */
typedef struct {
  uint64_t z_off, x_off;  /* stash byte offsets (block 0) of dZ and X slots */
  int32_t z_nt, x_nt;     /* tiles per block of the two slots */
  int32_t z_t0, x_t0;     /* first tile used */
  int32_t n_nt, n_kt;     /* n-tiles of dZ, k-tiles of X handled by this job */
  int32_t blk0, blk1;     /* block range [blk0, blk1) */
  int32_t w_off;          /* offset (floats) of the gradient matrix (row-major (out,in)) in the flat
                             gradient buffer, -1 = none */
  int32_t ld;
  int32_t r0, c0;         /* destination row / col of (tile 0, tile 0) */
  int32_t r_end, c_end;   /* valid bounds */
  int32_t b_off;          /* offset of the bias gradient or -1 (db[r] += sum_p dZ[p][r]) */
  int32_t pad;
  uint64_t x2_off;        /* second X slot: stash byte offset (block 0) */
  int32_t x2_nt, x2_t0;   /* its tiles per block, first tile used */
  int32_t n_kt1;          /* k-tiles taken from the first X slot (the remaining n_kt - n_kt1 from the second) */
  int32_t p_tile;         /* batched launches with HnDwBatch.partials (ABI 331): the job writes its n_nt x n_kt dW tiles —
                             raw accumulators, tile (i, j) at partials + (p_tile + i * n_kt + j) * 1024 floats, element
                             [register quad][lane][4]; bias sums in tile p_tile + n_nt * n_kt — with plain stores instead of adding them to the gradient by float
                             atomics; hn_mlp_wgrad_reduce sums the jobs' slabs and adds each element ONCE */
} HnDwJob;

int hn_version(void);
/* sizeof() of the ABI structs, in the order HnMlpArgs, HnPackUnit, HnPackBias, HnDwJob,
 * HnCompositeArgs, HnFeat, HnSlot, HnSrc — lets a foreign-language binding that keeps mirrors of its own verify them.
 * The Python binding keeps none: it derives every struct and every integer macro from this header's text when it is
 * imported, so the typedefs and #defines here stay in the plain forms that parser knows (one-dimensional arrays sized by
 * an integer or an earlier macro, macros that are integer literals). */
int hn_abi_sizes(int32_t* out, int n);
/* The build-time tuning knobs of THIS library (ABI 340): out[0..] = ring depth and LDS-DMA pieces per wave and stage of
 * hn_wgrad_kernel, bias-by-MFMA build, weight-stream chunk in units, block-read build, asymmetric weight-stream issue,
 * waves per workgroup of the bf16 machines, cache policy of the stash stream.  Entries 2, 4 and 5 are fixed at 0, 1 and 1
 * (those alternatives are no longer built); they keep their slots so that the layout stays the same.  Returns the number
 * of entries.  A binding derives its host-side mirrors (job stage cuts, chunk alignment, reduce tables) from these
 * instead of assuming the defaults. */
#define HN_BUILD_CONFIG_N 8
int hn_build_config(int32_t* out, int n);

/* Pack fp32 nn.Linear weights (row-major (out,in), reference layout hypernerf/modules.py:99-102)
 * into MFMA A-fragment order.  ptrs: device array of source pointers. */
int hn_pack_units(int mode, const HnPackUnit* units_dev, int n_units, const float* const* ptrs_dev,
                  void* wstream_dev, const HnPackBias* bias_dev, int n_bias, float* bias_out_dev,
                  hnStream_t stream);

/* The same for up to HN_MAX_PACK_JOBS programs in ONE launch (ABI 331): a training step re-packs the streams of three
 * programs after every optimizer step, and each of those launches costs more in dispatch than in work. */
#define HN_MAX_PACK_JOBS 8
typedef struct {
  const HnPackUnit* units;      /* device */
  const float* const* ptrs;     /* device: the program's pointer table */
  void* wstream;                /* device */
  const HnPackBias* bias;       /* device */
  float* bias_out;              /* device */
  int32_t n_units, n_bias;
} HnPackJob;
int hn_pack_units_multi(int mode, const HnPackJob* jobs_host, int n_jobs, hnStream_t stream);

int hn_mlp_forward(const HnMlpArgs* args, hnStream_t stream);
int hn_mlp_backward(const HnMlpArgs* args, hnStream_t stream);
/* Workspace query (host arithmetic only, no GPU needed): bytes of `stash` and of `masks` that the forward
 * (backward = 0) or backward (= 1) op program `ops_host` (HOST copy of HnMlpArgs.ops) touches for n_points
 * points in a training launch.  A stash is shared by a program's forward, backward and weight-gradient launches:
 * allocate the maximum of the two queries.  In the reference this is torch's autograd saving activations
 * (every nn.Linear / ReLU of hypernerf/modules.py:116-127). */
int hn_mlp_workspace_bytes(const int32_t* ops_host, int n_ops, int backward, int mode, int64_t n_points,
                           int64_t* stash_bytes, int64_t* mask_bytes);

/* dW/db for every Linear of a program: grads (fp32) are ACCUMULATED with float atomics.
 * `mode` of the three hn_mlp_wgrad* launches is a word: bits 0..7 = HN_MODE_*; HN_MODE_BF16_S8: bits 8.. = dz_scale_log2;
 * HN_MODE_BF16 / HN_MODE_F32: bits 8..15 = the LDS stage, in KiB, the host cut the jobs' blocks-per-stage (HnDwJob.pad
 * bits 16..23) for — 0 = not stated.  The kernel's ring is a compile-time constant of the library (2 x 64 KiB); a stated
 * stage that does not fit it is refused with -8 instead of silently loading part of every stage. */
int hn_mlp_wgrad(int mode, const HnDwJob* jobs_dev, int n_jobs, const void* stash_dev,
                 float* grad_base_dev, hnStream_t stream);

/* The same for up to HN_MAX_WGRAD_BATCH programs in ONE launch (a training step runs 6 programs; launched one by
 * one, the small ones cannot fill the chip and every launch pays its own ramp and tail).  Workgroup g works on job
 * g - first(batch) of the batch that holds it — or, with `order_dev` (device, one int32 per job of all batches:
 * batch << 24 | job), job order_dev[g]: the host's global heaviest-first order, which list-schedules 5 % tighter than
 * per-batch order.  `batches` is a HOST array, copied into the kernel arguments. */
#define HN_MAX_WGRAD_BATCH 8
typedef struct {
  const HnDwJob* jobs; /* device */
  const void* stash;   /* device: the stash the jobs' z_off / x_off refer to */
  float* grads;        /* device: base the jobs' w_off / b_off refer to */
  int32_t n_jobs;
  int32_t pad;
  float* partials;     /* device or NULL: workspace of the jobs' dW slabs (HnDwJob.p_tile), 4 KiB per tile; NULL = the
                          jobs add their tiles to `grads` themselves (float atomics) */
} HnDwBatch;
int hn_mlp_wgrad_batched(int mode, const HnDwBatch* batches_host, int n_batches, const int32_t* order_dev,
                         hnStream_t stream);
/* The same with a kernel timeline (HnMlpArgs.timeline; NULL = off). */
int hn_mlp_wgrad_batched_t(int mode, const HnDwBatch* batches_host, int n_batches, const int32_t* order_dev,
                           uint64_t* timeline_dev, hnStream_t stream);


/* Second half of a batched launch whose batches carry `partials` (ABI 331).  A job ends with the flush of its dW
 * rectangle; by float atomics one CU retires ~5 GB/s of them (one 256-B wave-instruction per ~50 ns), 100 us of a
 * 650-us launch at BASELINE config 2 during which the CU streams nothing.  With partials the jobs store their raw
 * accumulator tiles (plain 256-B stores) and this launch — one workgroup per DESTINATION tile (32 x 32 elements of
 * one gradient matrix) — sums the tile over every job that produced a slab for it, in the order of `list`, and adds
 * the sum to the gradient once: 1/12 of the atomics, and a summation order that does not depend on which job finished
 * first.  tiles_dev[t]: destination; its slabs are list_dev[first .. first + count): batch << 28 | slab tile index
 * (tile k of batch b starts at batches[b].partials + k * 1024 floats).  A record with ld == 0 is a BIAS record: w_off =
 * offset of the bias gradient, row0 = its first row, col0 = dZ tiles of the rectangle; a job with b_off >= 0 owns one
 * more slab tile behind its n_nt * n_kt dW tiles, 32 floats per dZ tile (HN_MODE_BF16_S8 keeps its bias atomics). */
typedef struct {
  int32_t batch;         /* whose `grads` receives the tile */
  int32_t w_off, ld;     /* gradient matrix (row-major (out, in)) in that buffer */
  int32_t row0, col0;    /* destination of accumulator element (row 0, col 0) of the tile */
  int32_t r_end, c_end;  /* valid bounds */
  int32_t first, count;  /* slice of list_dev */
} HnDwReduceTile;
/* Optional third kind of work of the same launch: the gradient of ONE gathered GLO table (modules.GLOEmbed's backward,
 * hypernerf/modules.py:155-167) from the per-block partial rows the backward machines of up to HN_MAX_WGRAD_BATCH
 * programs stored (HnMlpArgs.embed_partial): one workgroup per table row sums, program by program and block by block,
 * the rows of the blocks whose ray carries that index and adds the total to `grad` — a single writer per element, a
 * fixed order: with the slabs above the whole gradient of a step is bit-reproducible. */
typedef struct {
  float* grad;          /* (rows, dim) gradient of the table */
  int32_t rows, dim;
  uint32_t col_mask;    /* columns that carry a gradient (bit c = column c); dim <= 32 */
  int32_t n_src;
  const float* partial[HN_MAX_WGRAD_BATCH];   /* [n_blocks][dim] */
  const int64_t* idx[HN_MAX_WGRAD_BATCH];     /* ray -> table row */
  int32_t n_blocks[HN_MAX_WGRAD_BATCH];
  int32_t samples_per_ray[HN_MAX_WGRAD_BATCH];
} HnEmbedReduce;
int hn_mlp_wgrad_reduce(int mode, const HnDwReduceTile* tiles_dev, int n_tiles, const uint32_t* list_dev,
                        const HnDwBatch* batches_host, int n_batches, const HnEmbedReduce* embed_host,
                        hnStream_t stream);

/* The same launch, ALSO applying the optimizer (ABI 340; reference: train.py:116-131 configure_optimizers ->
 * utils.get_optimizer's torch.optim.Adam, utils/__init__.py:23-41, stepped right after loss.backward()): a workgroup
 * that has summed its destination tile updates the parameters behind it in registers (hn_adam_step's arithmetic,
 * operation for operation) and leaves the gradient buffer zeroed (zero_grad) or completed.  Single-GPU steps only: with an
 * all-reduce between backward and the optimizer the two-launch form stays.  `rest_dev`: the elements of the arena that
 * no tile / bias record / table row of this launch covers, as (start, len) ranges — each is handled by one more
 * workgroup, so that EVERY element of [0, n) is updated exactly once (the host builds and proves the partition).  All
 * `batches[i].grads` must be `grads`, the table gradient must lie inside [grads, grads + n): -9 otherwise. */
typedef struct {
  int64_t start;   /* first element (floats from the arena base) */
  int32_t len, pad;
} HnAdamRange;
typedef struct {
  float* params; float* grads; float* exp_avg; float* exp_avg_sq;   /* flat arena buffers of n floats, same layout */
  int64_t n;
  const float* hyper;   /* device: [lr, beta1, beta2, eps, weight_decay, grad_scale, -, -], as hn_adam_step */
  float* step;          /* device: [updates done, ticket], as hn_adam_step */
  const HnAdamRange* rest;   /* device */
  int32_t n_rest, zero_grad;
} HnAdamFuse;
int hn_mlp_wgrad_reduce_adam(int mode, const HnDwReduceTile* tiles_dev, int n_tiles, const uint32_t* list_dev,
                             const HnDwBatch* batches_host, int n_batches, const HnEmbedReduce* embed_host,
                             const HnAdamFuse* adam_host, hnStream_t stream);

/* ---- per-ray kernels --------------------------------------------------------------------- */

/* Stratified coarse samples + points.  model_utils.sample_along_rays (hypernerf/model_utils.py:6-41),
 * legacy models/rendering.py:189-207.  lower/upper: (n) per-bin bounds or (B,n) when per_ray_bounds;
 * t_rand (B,n) or NULL (z = lower).  Unfused fp32 ops in the reference's order (bit-exact z). */
int hn_sample_along_rays(const float* origins, const float* dirs, int ray_ld, const float* lower,
                         const float* upper, int per_ray_bounds, const float* t_rand, float scale,
                         int n_rays, int n, float* z_out, float* pts_out, hnStream_t stream);

/* Legacy nerf_pl sampling with per-ray near/far taken from columns 6,7 of the (B,>=8) ray rows
 * (models/rendering.py:189-207): z = near*(1-t)+far*t (or the disparity form), optional perturbation
 * z = lower + (upper-lower)*(scale*t_rand), pts = o + d*z.  t_vals / one_minus_t: (n) from the host. */
int hn_sample_legacy(const float* rays, int ray_ld, const float* t_vals, const float* one_minus_t,
                     int use_disp, const float* t_rand, float scale, int n_rays, int n, float* z_out,
                     float* pts_out, hnStream_t stream);

/* Stand-alone positional encoders: model_utils.posenc_orig (hypernerf/model_utils.py:234-246),
 * models/nerf.py:4-38 Embedding, and model_utils.posenc (:255-274, jax_cos=1: cos taken as
 * sin(x + 0.5*3.1415926)).  out = [x if identity][sin(f_k x), cos(f_k x)]_k, blocks of c channels.
 * Forward: out != NULL, g_out == NULL.  Backward: g_out != NULL, g_x receives d/dx. */
int hn_posenc(const float* x, int64_t n, int c, const float* freqs, int n_freqs, int identity, int jax_cos,
              float* out, const float* g_out, float* g_x, hnStream_t stream);

/* Softplus/relu density + alpha compositing.  model_utils.volumetric_rendering
 * (hypernerf/model_utils.py:43-107, 319-362) with NerfModel.query_template's noise+softplus
 * (hypernerf/models.py:485-491); legacy variant models/rendering.py:144-170.
 * variant 0 = hypernerf (softplus, last dist 1e7|1e-7, eps 1e-5 in cumprod, acc drops last sample)
 * variant 1 = legacy    (relu(sigma+noise), last dist 1e10, eps 1e-10, opacity = full sum)
 * variant 2 = hypernerf constants, `raw` is an already activated density (stand-alone
 *             model_utils.volumetric_rendering) */
typedef struct {
  int32_t variant, n_rays, n_samples, white_bg, sample_at_infinity, warped_ld;
  int32_t has_dust;     /* filter_sigma (models.py:35-63): drop densities below dust_threshold */
  float dust_threshold;
  const float* rgb;    /* (B,S,3) */
  const float* raw;    /* (B,S) raw density */
  const float* noise;  /* (B,S) standard-normal draws (or NULL); the kernel adds noise_scale * noise to the raw density
                          (model_utils.noise_regularize, model_utils.py:300-317: randn * noise_std) */
  const float* z;      /* (B,S) */
  const float* dirs;   /* (B,3) row stride ray_ld */
  int64_t ray_ld;
  const float* warped; /* (B,S,warped_ld) or NULL */
  float* out_rgb;      /* (B,3) */
  float* out_depth;    /* (B) */
  float* out_acc;      /* (B) */
  float* out_weights;  /* (B,S) */
  float* out_med_depth;  /* (B) or NULL */
  float* out_med_points; /* (B) or NULL */
  /* backward only */
  const float* g_rgb;     /* (B,3) or NULL */
  const float* g_depth;   /* (B) or NULL */
  const float* g_acc;     /* (B) or NULL */
  const float* g_weights; /* (B,S) or NULL */
  float* d_rgb;           /* (B,S,3) */
  float* d_raw;           /* (B,S) */
  const float* keep;      /* (B,S) 0/1 density mask (filter_sigma's bounding box) or NULL; forward and backward */
  float noise_scale;      /* noise_std; 1 for draws that arrive already scaled */
  int32_t split;          /* with `perm`: samples per ray held by part 0 (the rest, n_samples - split, by part 1) */
  /* A level evaluated in TWO parts (ABI 330; NULL perm = one part, everything above as before).  The fine level of
   * NerfModel.forward re-evaluates the coarse level's samples (hypernerf/models.py:752-768, model_utils.py:206-232:
   * sort(cat(z_coarse, z_new))); the warp field / hyper sheet results of those points already exist, so the host
   * evaluates the OLD samples (part 0: rgb, raw, warped — (B, split, .) in the coarse level's order) and the NEW
   * samples (part 1: rgb1, raw1, warped1 — (B, n_samples - split, .) in draw order) separately and composites them
   * through the merge permutation of hn_sample_pdf_split: sorted sample s of ray b is entry k = perm[b][s] of
   * cat(part 0, part 1) of that ray.  z, noise, keep, weights and g_weights stay in sorted order.  The backward writes
   * d_rgb / d_raw (part 0) and d_rgb1 / d_raw1 (part 1) in the parts' own order. */
  const int32_t* perm;    /* (B,S) int32 or NULL */
  const float* rgb1;      /* (B,S-split,3) */
  const float* raw1;      /* (B,S-split) */
  const float* warped1;   /* (B,S-split,warped_ld) or NULL */
  float* d_rgb1;          /* backward */
  float* d_raw1;          /* backward */
  float* out_warped;      /* forward, optional: (B,S,warped_ld) = the parts' warped rows in sorted order (the level's
                             `warped_points`, hypernerf/models.py:654-669) */
} HnCompositeArgs;
int hn_composite_forward(const HnCompositeArgs* a, hnStream_t stream);
int hn_composite_backward(const HnCompositeArgs* a, hnStream_t stream);

/* Median depth from given compositing weights: model_utils.compute_opaqueness_mask / compute_depth_index /
 * compute_depth_map (hypernerf/model_utils.py:319-362).  weights, z: (B, S) row-major.  Outputs (each may be NULL):
 * index (B) int64 = first sample whose inclusive weight sum reaches `threshold` (0 if none does: argmax of an
 * all-zero mask), depth (B) = z at that sample (0 if none), mask (B, S) = 1 at that sample, 0 elsewhere. */
int hn_depth_index(const float* weights, const float* z, int n_rays, int n_samples, float threshold,
                   int64_t* out_index, float* out_depth, float* out_mask, hnStream_t stream);

/* Inverse-CDF hierarchical sampling + merge-sort + points.  model_utils.piecewise_constant_pdf /
 * sample_pdf (hypernerf/model_utils.py:160-232) == legacy models/rendering.py:14-55,225-233.
 * weights: first used column of a (B, *) array with row stride w_ld, n_bins columns used;
 * bins: (B, n_bins+1) bin edges, or NULL = midpoints of z (then n_bins == n_coarse-2, and the caller
 * passes weights+1, i.e. coarse weights[:, 1:-1], as hypernerf/models.py:752-755 does);
 * z: (B, n_coarse) sorted coarse depths merged with the new samples, or NULL = no merge;
 * u: (B, n_fine).  Outputs (each may be NULL): z_all (B, n_coarse+n_fine) sorted, pts (.., 3),
 * inds (B, n_fine) int64 = searchsorted(cdf, u, right=True), z_samples (B, n_fine) unsorted.
 * The pdf normaliser is an fp64 sequential sum rounded once to fp32 and the cdf an fp64 sequential
 * prefix sum rounded per entry (== CPU torch.cumsum), so indices are bit-reproducible. */
int hn_sample_pdf(const float* weights, int w_ld, const float* bins, int n_bins, const float* z,
                  int n_coarse, const float* u, const float* origins, const float* dirs, int ray_ld,
                  int n_rays, int n_fine, float* z_all, float* pts, int64_t* inds, float* z_samples,
                  hnStream_t stream);
/* The same (ABI 330), for a fine level that evaluates only its NEW samples through the warp field (HnCompositeArgs.perm):
 * two more outputs, each may be NULL — perm (B, n_coarse+n_fine) int32: sorted position s holds entry perm[b][s] of
 * cat(z[b], z_samples[b]) (k < n_coarse: coarse sample k; else new sample k - n_coarse; equal depths keep that
 * order), and pts_new (B, n_fine, 3) = o + z_samples * d in draw order.  z_all / pts / inds / z_samples are bit-for-bit
 * those of hn_sample_pdf (the sort carries the index as a payload; keys are compared first).  perm needs z and z_all. */
int hn_sample_pdf_split(const float* weights, int w_ld, const float* bins, int n_bins, const float* z,
                        int n_coarse, const float* u, const float* origins, const float* dirs, int ray_ld,
                        int n_rays, int n_fine, float* z_all, float* pts, int64_t* inds, float* z_samples,
                        int32_t* perm, float* pts_new, hnStream_t stream);

/* A level's compositing (hn_composite_forward) AND the inverse-CDF sampling of the next level from its weights
 * (hn_sample_pdf_split's fused form: bins = midpoints of a->z, weights = columns 1 .. S-2 of the level's weights) as ONE
 * launch (ABI 340; reference call order models.py:744-768): the wave that composites a ray draws its fine samples, the
 * weights reach the sampler through LDS.  Outputs and arithmetic of both entry points, bit for bit; a->perm must be NULL. */
int hn_composite_sample_pdf(const HnCompositeArgs* a, const float* u, const float* origins, const float* dirs, int ray_ld,
                            int n_fine, float* z_all, float* pts, int64_t* inds, float* z_samples, int32_t* perm,
                            float* pts_new, hnStream_t stream);

/* GLO embedding lookup (modules.GLOEmbed, hypernerf/modules.py:155-167) and its gradient:
 * d_table[idx[b]] += sum_s d_embed[b, s, col0 : col0+dim]. */
int hn_embed_gather(const float* table, const int64_t* idx, int n_rays, int dim, int n_rows,
                    float* out, hnStream_t stream);
int hn_embed_backward(const float* d_points, int ld, int col0, const int64_t* idx, int n_rays,
                      int n_samples, int dim, int n_rows, float* d_table, hnStream_t stream);

/* Random draws of a render step in one launch (replaces the reference's torch.rand / torch.randn calls:
 * model_utils.py:31 t_rand, :226 u, :300-317 density noise).  Counter-based Philox4x32-10; state_dev = uint64[3]
 * {seed, offset, ticket (must start 0)} in device memory: the kernel advances `offset` itself, so a launch captured
 * in a HIP graph draws new numbers on every replay.  kind 0 = U[0,1) (24-bit, as torch.rand), 1 = N(0,1). */
#define HN_MAX_DRAWS 8
typedef struct HnDraw {
  float* ptr;      /* device buffer */
  int64_t n;       /* floats to fill */
  int32_t kind;
  int32_t pad;
} HnDraw;
int hn_random_fill(const HnDraw* draws_host, int n_draws, uint64_t* state_dev, hnStream_t stream);

/* The head of a render step as ONE launch (ABI 340): the weight streams of the step's programs (hn_pack_units_multi's
 * jobs), all its random draws (hn_random_fill's table and device state), the coarse samples placed from the t_rand draw
 * (hn_sample_along_rays: reference hypernerf/model_utils.py:6-41, same three separately rounded operations) and the int64
 * image ids of the (B, 9) ray rows (prepare_ray_dict's `rays[:, 8].type(torch.long)`, model_utils.py:365-404).  Any part
 * may be empty (n_pack = 0, n_draws = 0, p = NULL / t_rand_draw = -1 / n_ids = 0). */
typedef struct {
  int32_t t_rand_draw;     /* index into `draws` of the uniform (n_rays x n) buffer that is t_rand, or -1: no sampling */
  int32_t n_rays, n, ray_ld, per_ray_bounds;
  float scale;
  const float* origins; const float* dirs;   /* (n_rays, >= 3) rows, stride ray_ld */
  const float* lower; const float* upper;    /* (n) or (n_rays, n) bin bounds */
  float* z_out; float* pts_out;              /* (n_rays, n), (n_rays, n, 3) | NULL */
  const float* ids_src; int64_t* ids_dst;    /* ids_dst[i] = (int64) ids_src[i * ids_ld], i < n_ids */
  int32_t ids_ld, n_ids;
} HnPrologue;
int hn_render_prologue(int mode, const HnPackJob* pack_jobs_host, int n_pack, const HnDraw* draws_host, int n_draws,
                       uint64_t* state_dev, const HnPrologue* p_host, hnStream_t stream);


/* The reference's loss head (losses.py:4-14): loss = mean((coarse - gt)^2) [+ mean((fine - gt)^2)] over (B,3) pixels,
 * one launch forward (one workgroup; the result is written, not accumulated) and one launch backward:
 * d_coarse = d_fine-style 2 (pred - gt) / n * g_loss[0] (g_loss on the device; NULL = 1).  fine / d_fine may be NULL. */
int hn_mse_loss_forward(const float* coarse, const float* fine, const float* gt, int64_t n, float* loss_out,
                        hnStream_t stream);
int hn_mse_loss_backward(const float* coarse, const float* fine, const float* gt, int64_t n, const float* g_loss,
                         float* d_coarse, float* d_fine, hnStream_t stream);
/* Forward that also writes the gradients hn_mse_loss_backward would write for a root gradient of exactly 1 (bit for bit):
 * a training step whose loss is the root of the backward pass needs no second launch. */
int hn_mse_loss_forward_grad(const float* coarse, const float* fine, const float* gt, int64_t n, float* loss_out,
                             float* d_coarse, float* d_fine, hnStream_t stream);

/* SSIM of the reference's metrics.py:15-20 (kornia's ssim loss, `dssim`): per (n, c) plane the dissimilarity map
 * dssim = clamp((1 - S) / 2, 0, 1), S = ((2 mux muy + c1)(2 sxy + c2)) / ((mux^2 + muy^2 + c1)(sxx + syy + c2) + eps), the
 * moments filtered with the outer product of the 1-D window `window_host` (HOST array of `window` floats: kornia's
 * get_gaussian_kernel1d(window, 1.5)) over a reflect-padded image (F.pad mode='reflect').  pred / gt: fp32 (n, c, h, w)
 * with arbitrary element strides (`*_strides`: HOST arrays of 4).  window: odd, 3 .. 15; h and w > window / 2 (else -2).
 * hn_ssim_forward writes the map (dssim_map, contiguous, may be NULL) and/or the sum of the map over all n*c*h*w elements
 * (sum_out: ONE device float, written, not accumulated; may be NULL), the sum with per-workgroup partials in `workspace`
 * (hn_ssim_workspace_bytes: host arithmetic) and a second launch that adds them in a fixed order: bit-reproducible.
 * hn_ssim_backward: the upstream gradient is either g_scalar (ONE device float: every element of the map gets it) or
 * g_map (contiguous (n, c, h, w)), exactly one of them; d_pred (and d_gt unless NULL) are written, contiguous, as the
 * adjoint of the forward including the reflect padding. */
#define HN_SSIM_MAX_R 7 /* largest window radius: window sizes 3, 5, ..., 15 */
int hn_ssim_workspace_bytes(int n, int c, int h, int w, int window, int64_t* bytes);
int hn_ssim_forward(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int n,
                    int c, int h, int w, const float* window_host, int window, float c1, float c2, float eps,
                    float* dssim_map, float* sum_out, void* workspace, hnStream_t stream);
int hn_ssim_backward(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int n,
                     int c, int h, int w, const float* window_host, int window, float c1, float c2, float eps,
                     const float* g_scalar, const float* g_map, float* d_pred, float* d_gt, hnStream_t stream);

/* Multi-scale SSIM (the widely used NumPy `MultiScaleSSIM`, max_val folded into c1 / c2): a metric, no backward.  Five
 * levels; level 0 is the caller's pair pred / gt, fp32 (n, c, h, w) with arbitrary element strides (`*_strides`: HOST
 * arrays of 4), level l + 1 the 2 x 2 box mean of level l (out[i][j] = mean(in[2i..2i+1][2j..2j+1]), an index past the
 * edge replaced by the edge pixel, sides (h+1)/2 x (w+1)/2).  Per level the five moments are VALID correlations (no
 * padding, (h_l - size_l + 1) x (w_l - size_l + 1) outputs) with the outer product of the level's 1-D window:
 * taps_host = HOST array of 5 x 11 floats, row l holding sizes_host[l] taps; sizes_host = HOST array of 5 ints, each
 * 1 .. 11 and no larger than either side of its level (the metric uses min(11, h_l, w_l), sigma = size * 1.5 / 11, even
 * sizes sampled at half-integer offsets).  With s11 = E[xx] - mu1^2 etc., v1 = 2 s12 + c2, v2 = s11 + s22 + c2,
 *   levels_out[i][l][0] = mean(((2 mu1 mu2 + c1) v1) / ((mu1^2 + mu2^2 + c1) v2)),  levels_out[i][l][1] = mean(v1 / v2),
 * the means over all valid positions and all channels of image i; levels_out: (n, 5, 2) DEVICE floats, written.  The
 * product over the levels is left to the caller.  `workspace` (hn_msssim_workspace_bytes: host arithmetic) holds, in
 * floats, the planes of levels 1 .. 4 (per level the (n, c, h_l, w_l) first image, then the second), then per level
 * 0 .. 4 two partial sums per workgroup (one workgroup per 32 x 16 input tile of a plane); six launches, the last adds
 * the partial sums in a fixed order: no float atomics, bit-reproducible.  The host arrays are consumed at the call.
 * Status: -2 for every refused argument (n, c, h, w < 1, a NULL pointer, a size outside 1 .. 11 or above its level's
 * sides), checked before the first launch. */
#define HN_MS_LEVELS 5
#define HN_MS_MAX_SIZE 11 /* taps per row of taps_host; window sizes 1 .. 11 */
int hn_msssim_workspace_bytes(int n, int c, int h, int w, int64_t* bytes);
int hn_msssim_forward(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int n,
                      int c, int h, int w, const float* taps_host, const int* sizes_host, float c1, float c2,
                      float* levels_out, void* workspace, hnStream_t stream);

/* Geometry out of a trained field (csrc/hn_geometry.hip; no reference counterpart).
 *
 * Lattice: (nx, ny, nz) points, each side >= 2 and 7*nx*ny*nz <= 2^31 - 1, over bounds_host = HOST array
 * (xmin, xmax, ymin, ymax, zmin, zmax) with hi > lo.  Point index p = (i*ny + j)*nz + k, position
 * lo + (i, j, k) * step, step = (hi - lo) / (n - 1) in fp32 on the host, product and sum rounded on their own.
 *
 * hn_grid_points: out[r] = position of lattice point min(start + r, N - 1) for r < count — `count` points of the
 * lattice as (count, 3) fp32; indices past the lattice (the padding of a last chunk) repeat its last point.
 *
 * hn_density_activate: sigma[r] = softplus(raw[r]) (beta 1, threshold 20: as the compositing kernel takes it), then
 * filter_sigma: 0 where sigma < dust_threshold (has_dust != 0) or points[r] (n, 3) lies outside box_host = HOST array
 * (xmin, xmax, ymin, ymax, zmin, zmax), borders inside (box_host may be NULL: no box, points unused).
 *
 * Isosurface of the C-contiguous fp32 grid f[nx][ny][nz] at `iso` by marching tetrahedra; inside = f >= iso, NaN is
 * outside.  Cells are split into the six Kuhn tetrahedra around the main diagonal (q-th permutation pi of the axes in
 * lexicographic order: v0 = origin, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = v0 + (1,1,1)).  A vertex lies on a
 * tetrahedron edge and is named by the edge slot e = 7*p + d of the edge's LOWER lattice point p, d = the class of its
 * direction: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).  Workgroups are 256 points (or cells) each:
 * every *_blocks array has ceil(points / 256) (hn_iso_faces: ceil(cells / 256)) entries.
 *   hn_iso_mark      mask[p] = bit d set when the owned edge d exists and its ends differ in `inside`;
 *                    block_counts[b] = set bits of workgroup b.
 *   hn_iso_vertices  block_offsets = the exclusive scan of those counts (int64).  Vertex ids ascend with the edge slot.
 *                    For a = p, b = its neighbour, t = (iso - fa) / (fb - fa): vertices[id] = pos(a) + t*(pos(b) - pos(a)),
 *                    normals[id] = -g/|g|, g = ga + t*(gb - ga), ga / gb central differences of f at the two ends
 *                    (one-sided on the lattice boundary), (0,0,0) when |g| is 0 or NaN; every operation fp32, unfused.
 *                    slots[7*p + d] = id, or -1 for an edge without a vertex (all 7*N entries are written).
 *   hn_iso_faces     faces_dev == NULL: block_counts[b] = triangles of the cells of workgroup b (0, 1 or 2 per
 *                    tetrahedron).  Otherwise block_offsets = their exclusive scan (int64) and faces (F, 3) int32 is
 *                    written: by cell c = (i*(ny-1) + j)*(nz-1) + k, tetrahedron, triangle; vertex ids read from slots.
 *                    The winding comes from the inside mask and the sign of an integer determinant of lattice vectors:
 *                    normals point from inside to outside (towards lower f).
 * No atomics: the same grid gives the same arrays on every run.  Status: -2 for every refused argument (a NULL pointer
 * that must not be, a side < 2, 7*N above 2^31 - 1, hi <= lo, start / count outside the lattice), before any launch. */
#define HN_ISO_BLOCK 256 /* lattice points (hn_iso_faces: cells) per workgroup: the length of every *_blocks array */
int hn_grid_points(int nx, int ny, int nz, const float* bounds_host, long long start, long long count, float* out_dev,
                   hnStream_t stream);
int hn_density_activate(const float* raw_dev, const float* points_dev, long long n, int has_dust, float dust_threshold,
                        const float* box_host, float* sigma_dev, hnStream_t stream);
int hn_iso_mark(const float* grid_dev, int nx, int ny, int nz, float iso, uint8_t* mask_dev, int32_t* block_counts_dev,
                hnStream_t stream);
int hn_iso_vertices(const float* grid_dev, int nx, int ny, int nz, const float* bounds_host, float iso,
                    const uint8_t* mask_dev, const int64_t* block_offsets_dev, float* vertices_dev, float* normals_dev,
                    int32_t* slots_dev, hnStream_t stream);
int hn_iso_faces(const float* grid_dev, int nx, int ny, int nz, float iso, const int32_t* slots_dev,
                 const int64_t* block_offsets_dev, int32_t* block_counts_dev, int32_t* faces_dev, hnStream_t stream);

/* Connected components of an indexed triangle mesh, filtering by component, view directions for vertex colours
 * (csrc/hn_geometry.hip; no reference counterpart).  faces (F, 3) int32, V vertices, F and V at most 2^31 - 1.
 *
 * Two vertices are connected when a face holds both; the label of a vertex is the SMALLEST vertex id of its component (a
 * vertex no face references is its own component).  parent (V) int32 is the working array and, once a round changes
 * nothing, the labels.  flags: two device int32, [0] = error (a vertex id or label outside [0, V) was met; such a face is
 * skipped, nothing is written out of bounds), [1] = the number of the last round that lowered an entry of parent.
 *   hn_cc_init   parent[v] = v, flags[1] = 0, flags[0] = 1 when a face holds an id outside [0, V) (flags[0] is only ever
 *                set: the caller zeroes it).  F = 0 or V = 0 allowed (their pointers may then be NULL).
 *   hn_cc_round  round `round` >= 1, two launches.  hook: per face m = min of the parents of its three vertices,
 *                atomicMin(parent[x], m) for the three vertices and their three parents.  jump: per vertex follow parent
 *                for at most 16 hops (ids strictly decrease) and atomicMin the entry with where that got to.  Whatever
 *                lowered an entry stores `round` into flags[1]; the caller reads the flags after every round and stops at
 *                the first round r with flags[1] != r.  Invariant: parent[v] <= v and parent[v] lies in v's component, so
 *                the fixed point (every face sees one value, every parent is a root) is the smallest id whatever the
 *                scheduling; only integer atomicMin is used.  At most V - 1 rounds change something (each does at least a
 *                step of min-label propagation), one more reports none: the caller's cap is V + 1.
 *   hn_cc_sizes  sizes[labels[first vertex of f]] += 1 per face (sizes (V) int32, zeroed by the caller; integer
 *                atomicAdd: a workgroup of 2048 faces sends one add for the faces that carry the label of its first
 *                face, the lanes of a wave one add per other distinct label).
 *   hn_mesh_keep vkeep[v] = keep_comp[labels[v]] != 0, fkeep[f] = keep_comp[labels[first vertex of f]] != 0 as int32 0 / 1
 *                (keep_comp: V bytes indexed by label); a face with an id outside [0, V) is dropped.
 *   hn_mesh_compact  vscan / fscan = the inclusive scans (int32) of vkeep / fkeep, n_*_out their last entries:
 *                vertex_index[vscan[v] - 1] = v for a kept vertex; a kept face goes to row fscan[f] - 1 with every id
 *                replaced by vscan[id] - 1.  Relative orders are kept; no atomics.
 *   hn_gather_rows   dst[r] = src[index[r]] for r < n_rows, rows of row_bytes (<= 65536) bytes, index int32 in [0, n_src)
 *                (an index outside gives a zero row).
 *   hn_vertex_viewdirs  out[r] (count, 3) fp32 = u / |u| at vertex i = min(start + r, V - 1) (rows past the mesh, the
 *                padding of a last chunk, repeat the last vertex): u = -normals[i] when cam_host == NULL, else
 *                vertices[i] - cam_host[0..2] (HOST array); |u| = sqrt((ux*ux + uy*uy) + uz*uz), every operation fp32,
 *                unfused; |u| = 0 or NaN gives (0, 0, 1).
 * Status: -2 for every refused argument (a NULL pointer that must not be, a negative count, F or V above 2^31 - 1,
 * round < 1, start outside the mesh, count <= 0, n_*_out above its input), before any launch. */
int hn_cc_init(const int32_t* faces_dev, long long n_faces, int32_t* parent_dev, long long n_vertices, int32_t* flags_dev,
               hnStream_t stream);
int hn_cc_round(const int32_t* faces_dev, long long n_faces, int32_t* parent_dev, long long n_vertices, int round,
                int32_t* flags_dev, hnStream_t stream);
int hn_cc_sizes(const int32_t* labels_dev, const int32_t* faces_dev, long long n_faces, long long n_vertices,
                int32_t* sizes_dev, int32_t* flags_dev, hnStream_t stream);
int hn_mesh_keep(const int32_t* labels_dev, const int32_t* faces_dev, const uint8_t* keep_comp_dev, long long n_vertices,
                 long long n_faces, int32_t* vkeep_dev, int32_t* fkeep_dev, hnStream_t stream);
int hn_mesh_compact(const int32_t* faces_dev, const int32_t* vscan_dev, const int32_t* fscan_dev, long long n_vertices,
                    long long n_faces, long long n_vertices_out, long long n_faces_out, int32_t* vertex_index_dev,
                    int32_t* faces_out_dev, hnStream_t stream);
int hn_gather_rows(const void* src_dev, long long n_src, const int32_t* index_dev, long long n_rows, long long row_bytes,
                   void* dst_dev, hnStream_t stream);
int hn_vertex_viewdirs(const float* vertices_dev, const float* normals_dev, long long n_vertices, long long start,
                       long long count, const float* cam_host, float* out_dev, hnStream_t stream);

/* Mesh simplification by vertex clustering (csrc/hn_simplify.hip; DESIGN.md holds the definition, tests/simplify_restated.py
 * restates it in NumPy float32).  origin_host / cell_host: three HOST floats each, every cell side positive and finite.
 *   hn_simplify_extent     partial[6 b + 0 .. 2] / [6 b + 3 .. 5] = the per-axis minimum / maximum of the vertices 2048 b ..
 *                2048 b + 2047 (n_partial must be ceil(V / 2048)); NaN in all six when the tile holds a NaN.  The caller
 *                reduces the partials.
 *   hn_simplify_keys       keys[v] (int64) = ix | iy << 21 | iz << 42 with idx_c = floorf((v_c - origin_c) / cell_c), fp32,
 *                the subtraction and the division rounded on their own; an index outside [0, 2^21) is clamped (the caller
 *                checks the extent first).
 *   hn_simplify_reduce     one work-item per cluster c < n_clusters walks its members order[starts[c] .. starts[c + 1]) (order:
 *                the vertex ids sorted by key, stable; starts: C + 1 int32) and writes the representative: out_vertices
 *                (C, 3) = the sequential fp32 mean, or with quadric != 0 mean + adj(A) b / det(A) clamped into the cell box of
 *                cluster_keys[c] (A = sum n n^T + regularization * k * I, b = sum n (n . (p - mean)); no step unless det is
 *                finite and positive); out_normals (C, 3) = the normalised sequential sum (zero when its length is not > 0;
 *                normals_dev may be NULL when quadric == 0: then no normals are written); colours by color_kind: 0 none,
 *                1 uint8 (C, 3) = (2 * sum + k) / (2 k) in integers, 2 fp32 (C, 3) = sequential sum / k.
 *   hn_simplify_face_keys  per face through vertex_cluster (V int32): rotated so that the smallest cluster id a comes first,
 *                (a, x, y) -> key_ab = a << 31 | min(x, y) (int64), key_c = max(x, y), sign = +1 when x < y, else -1; a face
 *                with two equal ids, an id outside [0, V) or a cluster id below 0: key_ab = 2^63 - 1, key_c = 2^31 - 1, sign 0.
 *   hn_simplify_face_net   over the faces sorted by (key_ab, key_c): sorted_ab[i] = key_ab[perm[i]], perm int64; key_c and sign
 *                are read through perm.  net[i] = the sum of the signs of the group of equal names that ENDS at i, 0 elsewhere.
 *   hn_simplify_face_emit  ends = the inclusive scan (int64) of |net|, n_out its last entry: the group that ends at i writes
 *                |net[i]| rows (a, b, c) (net > 0) or (a, c, b) (net < 0) at ends[i] - |net[i]| and stores 1 into used[a], used[b],
 *                used[c] (used: C int32 zeroed by the caller; plain stores of the same value, no atomics).
 *   hn_simplify_relabel    out[v] = scan[vertex_cluster[v]] - 1 when that cluster is used, else -1 (scan = inclusive scan of used).
 * Status: -2 for every refused argument (a NULL pointer that must not be, a count <= 0 or above 2^31 - 1, n_clusters above
 * n_vertices, n_out above n_faces, a cell side that is not positive and finite), before any launch. */
#define HN_EXTENT_TILE 2048  /* vertices per workgroup of hn_simplify_extent: n_partial = ceil(V / HN_EXTENT_TILE) */
#define HN_SIMPLIFY_BITS 21  /* bits per axis of a cell key (hn_simplify_keys) */
int hn_simplify_extent(const float* vertices_dev, long long n_vertices, float* partial_dev, long long n_partial,
                       hnStream_t stream);
int hn_simplify_keys(const float* vertices_dev, long long n_vertices, const float* origin_host, const float* cell_host,
                     int64_t* keys_dev, hnStream_t stream);
int hn_simplify_reduce(const float* vertices_dev, const float* normals_dev, const void* colors_dev, int color_kind,
                       const int32_t* order_dev, const int32_t* starts_dev, const int64_t* cluster_keys_dev,
                       long long n_clusters, long long n_vertices, const float* origin_host, const float* cell_host,
                       float regularization, int quadric, float* out_vertices_dev, float* out_normals_dev,
                       void* out_colors_dev, hnStream_t stream);
int hn_simplify_face_keys(const int32_t* faces_dev, long long n_faces, const int32_t* vertex_cluster_dev, long long n_vertices,
                          int64_t* key_ab_dev, int32_t* key_c_dev, int32_t* sign_dev, hnStream_t stream);
int hn_simplify_face_net(const int64_t* sorted_ab_dev, const int32_t* key_c_dev, const int32_t* sign_dev,
                         const int64_t* perm_dev, long long n_faces, int32_t* net_dev, hnStream_t stream);
int hn_simplify_face_emit(const int64_t* sorted_ab_dev, const int32_t* key_c_dev, const int64_t* perm_dev,
                          const int32_t* net_dev, const int64_t* ends_dev, long long n_faces, long long n_clusters,
                          long long n_out, int32_t* faces_out_dev, int32_t* used_dev, hnStream_t stream);
int hn_simplify_relabel(const int32_t* vertex_cluster_dev, long long n_vertices, const int32_t* used_dev,
                        const int32_t* scan_dev, long long n_clusters, int32_t* out_dev, hnStream_t stream);

/* Mesh rendering by ray casting (csrc/hn_mesh_render.hip; DESIGN.md 3.11 holds the definition, tests/mesh_render_restated.py
 * restates it in NumPy float32).  Pixel p of the H x W image has the ray (o, d) = rays[p * ray_ld + 0 .. 5]; cam_dev is the
 * 24-float camera record of hn_generate_rays_nerfies, on the device.  Vertices (V, 3) fp32, faces (F, 3) int32.
 *   hn_mesh_project    per vertex the forward camera model (rotate, divide, distort in closed form, intrinsics): pix (V, 2)
 *                fp32 pixel coordinates (pixel (i, j) covers [i, i + 1) x [j, j + 1)), flags (V) int32: 1 when z <= 1e-6 in the
 *                camera frame, 2 when 1 + 3 k1 r + 5 k2 r^2 + 7 k3 r^3 <= 0 at r = x^2 + y^2 (the radial map folds) or a
 *                coordinate is not finite; pix is (0, 0) under a flag.
 *   hn_mesh_bin_count  counts[f] (int32) = the 16 x 16 tiles in the box of face f: the box of its three projected vertices and
 *                three projected edge midpoints, padded by 1 pixel (+ 1/8 of its larger side when the camera has distortion),
 *                clipped to the image; the whole image when a vertex or midpoint has a flag; nothing when all three
 *                vertices have flag 1.  A face with an id outside [0, V) counts 0 and stores 1 into err[0] (int32, zeroed by
 *                the caller).
 *   hn_mesh_bin_fill   ends = the inclusive scan (int64) of counts, n_pairs its last entry: face f writes its (tile, face)
 *                pairs, tiles row by row (tile = ty * ceil(W / 16) + tx), to the rows ends[f] - counts[f] .. ends[f] - 1 of
 *                pair_tile / pair_face (int32).  A row outside [0, n_pairs) is not written.
 *   hn_mesh_trace      one workgroup per tile, one thread per pixel; tile T tests the faces pair_face[tile_begin[T] ..
 *                tile_end[T]) (int64 bounds, clamped to [0, n_pairs]), 64 at a time through LDS, and writes face (H*W int32, -1
 *                for none), depth (H*W fp32, the ray parameter t, 0 for none) and bary (H*W, 3 fp32, zeros for none) of the
 *                nearest hit, equal t going to the smaller face id.  A pair entry outside [0, F) or a vertex id outside
 *                [0, V) is skipped.  n_pairs may be 0 (pair_face, faces, vertices may then be NULL): an all-empty image.
 *   hn_mesh_shade      per pixel from face / bary: normal_out (H*W, 3) = the normalised interpolated vertex normal (normals_dev
 *                NULL: the face normal), rgb_out (H*W, 3) fp32 = clamp(colour * k, 0, 1) with the interpolated vertex colour
 *                (color_kind 1: uint8 / 255, 2: fp32, 0: base_color_host) and k = ambient + (1 - ambient) |N . d| (headlight
 *                != 0) or 1, rgb8_out = floor(255 rgb + 0.5); a pixel without a face: normal 0, background_host.
 *                base_color_host / background_host: three HOST floats in [0, 1]; ambient in [0, 1].
 * Status, before any launch: -2 for a size out of range (a count <= 0 where one is needed or above 2^31 - 1, an image side
 * outside 1 .. 65535, ray_ld < 6, a colour outside [0, 1]), -3 for a NULL pointer that must not be. */
#define HN_MESH_TILE 16        /* pixels per tile side: one workgroup of 256 threads per tile, one thread per pixel */
#define HN_MESH_MAX_SIDE 65535 /* image sides: pixel and tile coordinates stay exact in fp32 */
int hn_mesh_project(const float* vertices_dev, long long n_vertices, const float* cam_dev, float* pix_dev, int32_t* flags_dev,
                    hnStream_t stream);
int hn_mesh_bin_count(const int32_t* faces_dev, long long n_faces, const float* vertices_dev, const float* pix_dev,
                      const int32_t* vflags_dev, long long n_vertices, const float* cam_dev, int H, int W,
                      int32_t* counts_dev, int32_t* err_dev, hnStream_t stream);
int hn_mesh_bin_fill(const int32_t* faces_dev, long long n_faces, const float* vertices_dev, const float* pix_dev,
                     const int32_t* vflags_dev, long long n_vertices, const float* cam_dev, int H, int W,
                     const int64_t* ends_dev, long long n_pairs, int32_t* pair_tile_dev, int32_t* pair_face_dev,
                     hnStream_t stream);
int hn_mesh_trace(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                  const float* rays_dev, int ray_ld, int H, int W, const int64_t* tile_begin_dev,
                  const int64_t* tile_end_dev, const int32_t* pair_face_dev, long long n_pairs, int32_t* face_out_dev,
                  float* depth_out_dev, float* bary_out_dev, hnStream_t stream);
int hn_mesh_shade(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                  const float* normals_dev, const void* colors_dev, int color_kind, const float* rays_dev, int ray_ld,
                  long long n_pixels, const int32_t* face_dev, const float* bary_dev, int headlight, float ambient,
                  const float* base_color_host, const float* background_host, float* normal_out_dev, float* rgb_out_dev,
                  uint8_t* rgb8_out_dev, hnStream_t stream);

/* Depth fusion (csrc/hn_fusion.hip; DESIGN.md 3.12 holds the definition, tests/tsdf_restated.py restates it in NumPy float32).
 * The lattice is hn_grid_points' (nx, ny, nz over bounds_host, six HOST floats); cams_dev holds 24-float camera records of
 * hn_generate_rays_nerfies, on the device.
 *   hn_tsdf_integrate  folds depths (n_views, H, W) fp32 seen through cams (n_views, 24) into tsdf and weight, both (nx, ny, nz)
 *                fp32, z fastest, zeroed by the caller before the first batch (later batches continue them).  A depth is the
 *                distance along the unit ray from the camera position; +inf: the ray hit nothing (everything along it is
 *                free); a value that is not > 0 (zero, negative, NaN): nothing is known.  One work-item per lattice point x
 *                (the position hn_grid_points gives it, bit for bit) walks the views in order 0 .. n_views - 1; every
 *                operation is fp32, rounded on its own, in this order:
 *                  q = x - cam[9:12];  (u, v, flag) = the forward camera model of hn_mesh_project;  flag != 0 skips the view
 *                  skip unless 0 <= u < W and 0 <= v < H, compared as floats;  col = (int)floorf(u), row = (int)floorf(v)
 *                  D = depths[view][row][col];  skip unless D > 0
 *                  r = sqrt((qx*qx + qy*qy) + qz*qz);  s = D - r;  skip if s < -trunc
 *                  t = fminf(1, s / trunc);  tsdf = (weight * tsdf + t) / (weight + 1);  weight = weight + 1
 *                No atomics, no reductions: two runs, and the same views in several batches, give the same bits.
 *   hn_tsdf_face_keep  for a mesh extracted on that lattice (faces (F, 3) int32, vertices (V, 3) fp32) and the weight volume:
 *                fkeep[f] (int32) = 1 iff all eight lattice points of the cell that holds the face's centroid have weight > 0,
 *                centroid = ((a + b) + c) / 3 per axis, cell index per axis = min(n - 2, max(0, (int)floorf((centroid - lo) /
 *                step))) with step = (hi - lo) / (n - 1) as hn_grid_points takes it; a face with an id outside [0, V): 0.
 *                vkeep[v] (int32, V entries zeroed by the caller) = 1 iff a kept face references v (plain stores of the
 *                same value, no atomics).  Both are what hn_mesh_compact takes after two inclusive scans.
 * Status, before any launch: -2 for a size out of range (a lattice hn_grid_points refuses, n_views < 1, an image side outside
 * 1 .. 65535, trunc not positive and finite, F or V <= 0 or above 2^31 - 1, bounds_host NULL), -3 for a NULL device pointer. */
int hn_tsdf_integrate(float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const float* bounds_host,
                      const float* cams_dev, const float* depths_dev, int n_views, int H, int W, float trunc,
                      hnStream_t stream);
int hn_tsdf_face_keep(const int32_t* faces_dev, long long n_faces, const float* vertices_dev, long long n_vertices,
                      const float* weight_dev, int nx, int ny, int nz, const float* bounds_host, int32_t* fkeep_dev,
                      int32_t* vkeep_dev, hnStream_t stream);

/* Empty-space skipping (csrc/hn_occupancy.hip; DESIGN.md 3.18 holds the definition, tests/occupancy_restated.py restates it
 * in NumPy).  A lattice of (nx, ny, nz) points, as hn_grid_points lays it out, has (cx, cy, cz) = (nx-1, ny-1, nz-1) cells;
 * their occupancy is (cx, cy, words) uint64 with words = ceil(cz / 64): bit b of word w of row (i, j) is cell
 * (i, j, 64 w + b), the bits past cz are zero.  At most 2048 cells per axis.
 *   hn_occ_mark       bits of the density lattice grid (nx, ny, nz) fp32: a cell is occupied iff one of its 8 corners is
 *                     >= sigma_min or NaN.  One wave writes one word (a 64-bit ballot): no atomics, the same bits every run.
 *   hn_occ_dilate     out = in dilated once by the 3 x 3 x 3 cube (26 neighbours).  Bits carry across word boundaries,
 *                     nothing wraps at the faces of the grid, the padding bits stay zero.  Not in place.
 *   hn_occ_count      *count (int64, on the device) = the number of set bits of n_words words (zeroed by a memset node on
 *                     the stream, then integer atomics: the sum does not depend on their order).
 *   hn_occ_clip_rays  rays (n, ray_ld >= 6) fp32 rows [o, d, ...]: the ray's part of [t_near, t_far] from the entry of the
 *                     first to the exit of the last occupied cell it crosses, by a 3-D DDA over the cells of bounds_host
 *                     (six HOST floats), one ray per work-item, at most cx + cy + cz + 3 steps.  Every plane distance is
 *                     ((lo + i * cell) - o) / d from the plane's index, each operation rounded on its own in fp32.  Space
 *                     outside the box is empty; a ray that is not finite, misses the box or meets no occupied cell is a
 *                     miss.  clip_far == 0 keeps t1 = t_far; an interval shorter than min_span grows by half the
 *                     difference at both ends, clamped to [t_near, t_far].  Outputs, each may be NULL: t (n, 2) = (t0, t1);
 *                     hit (n) uint8; rays_out (n, ray_ld): columns 0-2 o + d * a, 3-5 b * d with
 *                     b = (t1 - t0) / (t_far - t_near), a = t0 - b * t_near, the other columns copied; affine (n, 2) = (a, b),
 *                     so that a model sampling z in [t_near, t_far] along the new row is at distance a + b z along the
 *                     old one.  A miss gives t = (t_near, t_far), hit 0, affine (0, 1) and the input row bit for bit, and so
 *                     does every row with t0 == t_near and t1 == t_far.
 *   hn_occ_clip_batch the same clip for a training batch that mixes frames, one launch, graph-capturable:
 *                     bits (n_slots, cx, cy, words) is a stack of grids that share cells and bounds_host; the id v of a ray
 *                     is column id_col of its row (id_col < 0: every ray has id 0; else 6 <= id_col < ray_ld); when v is
 *                     finite and 0 <= (int)v < n_ids its slot is slot_of_id[(int)v] (int32, on the device).  A slot
 *                     outside [0, n_slots), and any other v (NaN included), means "no grid": the row is copied, hit = 0,
 *                     affine = (0, 1).  With a slot, hit, affine and the output row are bit for bit those of
 *                     hn_occ_clip_rays on that slot's grid; with clip_far == 0 the walk ends at the first occupied cell
 *                     (t1 = t_far whatever lies behind it).  Every pointer read is fixed: a replayed graph sees what the
 *                     host wrote into bits and slot_of_id since.  Outputs, each may be NULL: rays_out (n, ray_ld), not
 *                     rays; viewdirs_out (n, 3) = the INPUT rows' d; affine (n, 2); hit (n) uint8; hit_count (int64, on the
 *                     device) = the number of hits, zeroed by a one-lane launch on the stream, then one integer atomic
 *                     per wave: the same number on every run.
 * Status, before any launch: -2 for a size out of range (no cell or more than 2048 along an axis, a lattice hn_grid_points
 * refuses, hi <= lo or a bound that is not finite, a NaN sigma_min, n or n_words outside 1 .. 2^31 - 1, ray_ld outside
 * 6 .. 64, t_far <= t_near or not finite, min_span negative or not finite, bounds_host NULL, out == in, id_col in 0 .. 5 or
 * >= ray_ld, n_slots or n_ids < 1), -3 for a NULL device pointer that must not be. */
int hn_occ_mark(const float* grid_dev, int nx, int ny, int nz, float sigma_min, uint64_t* bits_dev, hnStream_t stream);
int hn_occ_dilate(const uint64_t* in_dev, uint64_t* out_dev, int cx, int cy, int cz, hnStream_t stream);
int hn_occ_count(const uint64_t* bits_dev, long long n_words, int64_t* count_dev, hnStream_t stream);
int hn_occ_clip_rays(const float* rays_dev, long long n, int ray_ld, const uint64_t* bits_dev, int cx, int cy, int cz,
                     const float* bounds_host, float t_near, float t_far, int clip_far, float min_span, float* t_dev,
                     uint8_t* hit_dev, float* rays_out_dev, float* affine_dev, hnStream_t stream);
int hn_occ_clip_batch(const float* rays_dev, long long n, int ray_ld, int id_col, const uint64_t* bits_dev, int n_slots,
                      int cx, int cy, int cz, const int32_t* slot_of_id_dev, int n_ids, const float* bounds_host,
                      float t_near, float t_far, int clip_far, float min_span, float* rays_out_dev,
                      float* viewdirs_out_dev, float* affine_dev, uint8_t* hit_dev, int64_t* hit_count_dev,
                      hnStream_t stream);

/* Mesh-to-mesh distance (csrc/hn_mesh_distance.hip; DESIGN.md 3.13 holds the definition, tests/mesh_distance_restated.py
 * restates it in NumPy float32).  Vertices (V, 3) fp32, faces (F, 3) int32; every fp32 operation that decides a result is
 * rounded on its own, dot(u, v) = (ux*vx + uy*vy) + uz*vz.  lo_host / cell_host: three HOST floats each, the low corner
 * and the cell sides of a grid of rx x ry x rz cells (1 .. 256 each: a cell index fits 24 bits, a face's cell count an
 * int32); idx_c(x) = floorf((x - lo_c) / cell_c) clamped to [0, R_c - 1], a NaN giving 0; cell = (iz * ry + iy) * rx + ix.
 *   hn_md_face_weights  a2[f] = |(B - A) x (C - A)|, twice the area: each component of the cross product one product minus
 *                another, the length sqrt(dot(n, n)); 0 unless finite.  A face with an id outside [0, V) gets 0 and stores 1
 *                into err[0] (int32, zeroed by the caller).
 *   hn_md_sample        sample k < n of the surface: h_j = splitmix64(key + 3 k + j), key = splitmix64(seed) (64-bit wrap-around);
 *                t = the high 64 bits of h_0 * W with W = cdf[F - 1]; face = the first f with cdf[f] > t (cdf (F) int64: the
 *                inclusive scan of the caller's integer weights, W > 0); u1 = (h_1 >> 40) * 2^-24, u2 likewise from h_2;
 *                s = sqrt(u1); bary (n, 3) = (1 - s, s * (1 - u2), s * u2); points (n, 3) = (b0*A + b1*B) + b2*C per
 *                coordinate (NaN when the face holds an id outside [0, V)); face (n) int32.
 *   hn_md_pack          tri (F, 12) fp32 = A, B, C and three zeros of padding, so that a candidate is three
 *                16-byte loads and no index; NaN in all nine for a face with an id outside [0, V), which stores 1 into err[0].
 *   hn_md_cell_count    counts[f] (int32) = the cells of [idx(min corner), idx(max corner)] of packed triangle f, 0 when it
 *                holds a NaN.
 *   hn_md_cell_fill     ends = the inclusive scan (int64) of counts, n_pairs its last entry: face f writes its (cell, face)
 *                pairs, x fastest, to the rows ends[f] - counts[f] .. ends[f] - 1 of pair_cell / pair_face (int32).  A row
 *                outside [0, n_pairs) is not written.
 *   hn_md_cell_keys     keys[i] (int32) = the cell of query point i (the key the caller sorts the queries by).
 *   hn_md_query         one work-item per query slot j < n: point i = perm[j] (perm (n) int64, NULL: i = j; an entry outside
 *                [0, n) is skipped) gets the lexicographic minimum of (d2, face id) over the faces with d2 < +inf, d2 the
 *                squared distance to the closest point of the triangle by Voronoi regions (operation order: DESIGN.md 3.13):
 *                distance (n) fp32 = sqrt(d2), face (n) int32, closest (n, 3) fp32; +inf, -1, NaN without such a face; NaN,
 *                -1, NaN for a point that is not finite.  The faces of cell c are pair_face[cell_begin[c] .. cell_begin[c +
 *                1]) (cell_begin: rx * ry * rz + 1 int32, clamped to [0, n_pairs]; an entry of pair_face outside [0, F) is
 *                skipped).  The walk goes through Chebyshev shells of cells around the point's cell and stops when every
 *                cell was visited or no unvisited face can come closer: the result is that of testing every face.
 *                max_distance >= 0: a result with distance > max_distance becomes +inf, -1, NaN and the walk may stop at
 *                that radius; max_distance < 0: no limit.
 * Status, before any launch: -2 for a size out of range (a count <= 0 or above 2^31 - 1, a resolution outside 1 .. 256,
 * a cell side that is not positive and finite, a NaN max_distance), -3 for a NULL pointer that must not be. */
int hn_md_face_weights(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                       float* a2_dev, int32_t* err_dev, hnStream_t stream);
int hn_md_sample(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                 const int64_t* cdf_dev, long long n, long long seed, float* points_dev, int32_t* face_dev, float* bary_dev,
                 hnStream_t stream);
int hn_md_pack(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces, float* tri_dev,
               int32_t* err_dev, hnStream_t stream);
int hn_md_cell_count(const float* tri_dev, long long n_faces, const float* lo_host, const float* cell_host, int rx, int ry,
                     int rz, int32_t* counts_dev, hnStream_t stream);
int hn_md_cell_fill(const float* tri_dev, long long n_faces, const float* lo_host, const float* cell_host, int rx, int ry,
                    int rz, const int64_t* ends_dev, long long n_pairs, int32_t* pair_cell_dev, int32_t* pair_face_dev,
                    hnStream_t stream);
int hn_md_cell_keys(const float* points_dev, long long n, const float* lo_host, const float* cell_host, int rx, int ry, int rz,
                    int32_t* keys_dev, hnStream_t stream);
int hn_md_query(const float* points_dev, long long n, const int64_t* perm_dev, const float* tri_dev, long long n_faces,
                const int32_t* cell_begin_dev, const int32_t* pair_face_dev, long long n_pairs, const float* lo_host,
                const float* cell_host, int rx, int ry, int rz, float max_distance, float* distance_dev, int32_t* face_dev,
                float* closest_dev, hnStream_t stream);

/* Mesh registration (csrc/hn_registration.hip; DESIGN.md 3.15 holds the definition, tests/registration_restated.py restates
 * it in NumPy, bit for bit): the two kernels of an ICP iteration around hn_md_query.
 *   hn_reg_transform    out (n, 3) fp32 = s * (R p) + t for points (n, 3) fp32; params_host: 13 HOST floats, R row-major (9),
 *                s, t (3), all finite.  Every fp32 operation is rounded on its own: row_i = (R_i0*x + R_i1*y) + R_i2*z,
 *                out_i = row_i * s + t_i.  direction = 1: no s, no t, out = row / sqrtf(dot(row, row)), row itself unless
 *                the length is > 0 (a zero vector stays zero).  A point that is not finite gives NaN, NaN, NaN.
 *   hn_reg_moments      the sums one iteration solves from, over the inliers of points (n, 3) fp32 with hn_md_query's closest
 *                (n, 3), distance (n) and face (n): point k is an inlier when distance[k] is finite and <= tau[0] (one
 *                DEVICE fp32), 0 <= face[k] < n_faces and, with mode 1, the packed triangle tri[face[k]] (tri (F, 12) fp32
 *                of hn_md_pack) has a normal of positive finite length; nothing else is read into a sum.  Doubles from
 *                the fp32 inputs, every double operation rounded on its own, dot(u, v) = (ux*vx + uy*vy) + uz*vz.
 *                mode 0 (point to point), 19 values: count, sum d^2, sum p (3), sum q (3), sum q_i p_j (9, index 3 i + j),
 *                sum dot(p, p), sum dot(q, q).  mode 1 (point to plane), 38 values: count, sum d^2, sum r^2, the upper
 *                triangle of J^T J by rows (28), J^T r (7), with n = m / sqrt(dot(m, m)), m = (B - A) x (C - A),
 *                r = dot(p - q, n), J = [p x n, n, dot(p, n)].  sums (38) doubles, the unused tail 0; partials
 *                (n_blocks, 38) doubles of workspace.  n_blocks workgroups (1 .. 1024) of 256 threads: a thread adds its
 *                points k = g, g + 256 n_blocks, ... in order, a wave folds its lanes by halves, a workgroup adds its
 *                waves as (w0 + w1) + (w2 + w3), a second launch adds the partials in block order.  No atomics: the
 *                result is a function of the inputs, n and n_blocks, the same bits on every run.
 * Status, before any launch: -2 for a size out of range (n or n_faces <= 0 or above 2^31 - 1, n_blocks outside 1 .. 1024, a
 * mode or direction that is neither 0 nor 1, params_host NULL or not finite), -3 for a NULL device pointer that must not be
 * (tri may be NULL with mode 0). */
int hn_reg_transform(const float* points_dev, long long n, const float* params_host, int direction, float* out_dev,
                     hnStream_t stream);
int hn_reg_moments(const float* points_dev, const float* closest_dev, const float* distance_dev, const int32_t* face_dev,
                   long long n, const float* tri_dev, long long n_faces, const float* tau_dev, int mode, int n_blocks,
                   double* partials_dev, double* sums_dev, hnStream_t stream);

/* Texture atlas (csrc/hn_texture.hip; DESIGN.md 3.16 holds the definition, tests/texture_restated.py restates it in NumPy
 * float32): one chart per face, two faces to a square cell of power-of-two side s (16 .. 1024), cells packed in Z-order.
 * Vertices (V, 3) fp32, faces (F, 3) int32; every fp32 operation rounded on its own.  L = s - 7.
 *   hn_tex_classify   per face: class[f] (int32) = log2(s) of the smallest s in [min_cell, max_cell] with m <= (L*texel)^2, m the
 *                largest squared edge length ((dx*dx + dy*dy) + dz*dz); max_cell when none does.  keys[f] (int64) =
 *                (10 - class) << 32 | f: ascending keys are descending sides, ascending face ids.  A face with an id outside
 *                [0, V) gets min_cell and stores 1 into err[0] (int32, zeroed by the caller).
 *   hn_tex_layout     from the sorted keys: class_rank_host = 8 HOST int64, the first sorted rank of side 1024 >> q for q = 0 ..
 *                6, then F.  Side s with ranks r0 .. r1 has ceil((r1 - r0) / 2) cells, cell j holding rank r0 + 2j (lower
 *                half) and r0 + 2j + 1 (upper half, -1 past r1); cells are numbered side by side in that order, n_cells in
 *                all, and the Morton index of a cell is the sum of (side / min_cell)^2 over the cells before it: x from
 *                its even bits, y from its odd bits, times min_cell = cell_start (n_cells, 2) int32.  cell_side (n_cells)
 *                int32, cell_face (n_cells, 2) int32.  uv (F, 3, 2) fp32, absolute texel coordinates with texel (i, j)
 *                centred at (i + 0.5, j + 0.5): the lower half's corners at start + (1.5, 1.5), + (1.5 + L, 1.5), + (1.5,
 *                1.5 + L), the upper half's at the point mirror (x, y) -> (s - x, s - y) of those.
 *   hn_tex_rasterize  one work-item per texel of the (H, W) atlas (sides multiples of min_cell, at most 16384);
 *                class_cells_host = 8 HOST int64, the first cell of side 1024 >> q, then n_cells.  owner (H, W) int32 = the
 *                face of the half the texel lies in: the lower half owns i + j <= s - 2 (cell-relative), the upper half
 *                i + j >= s, nobody i + j = s - 1; -1 there, outside every cell, in an empty half and for a face or
 *                vertex id out of range.  position (H, W, 3) fp32 = (b0*v0 + b1*v1) + b2*v2 with b1 = (x - 1.5) / L,
 *                b2 = (y - 1.5) / L, b0 = (1 - b1) - b2 at the texel centre (x, y), mirrored first in the upper half; not
 *                clamped to the triangle.  normal (H, W, 3) fp32 = the vertex normals mixed alike and divided by their
 *                length sqrt(dot(N, N)) (normals_dev NULL, or a length not > 0: the face normal cross(v1 - v0, v2 - v0)
 *                alike; zero when that has no length either).  Unowned texels get zeros.
 *   hn_tex_shade      hn_mesh_shade with the colour from a texture (tex_h, tex_w, 3), texture_kind 1: uint8 / 255, 2: fp32:
 *                (u, v) = (w0*uv[f][0] + w1*uv[f][1]) + w2*uv[f][2] per coordinate, clamped to the bounding box of the three;
 *                filter 1 (bilinear): a = u - 0.5, i0 = floor(a), fx = a - i0, rows alike, top = c00 + fx*(c10 - c00), bot =
 *                c01 + fx*(c11 - c01), colour = top + fy*(bot - top); filter 0: the texel (floor(u), floor(v)).  Indices are
 *                clamped into the texture.  Normal, headlight factor, clamp to [0, 1], rgb8 and background as hn_mesh_shade.
 * Status, before any launch: -2 for a size out of range (a count <= 0 where one is needed or above 2^31 - 1, a cell side
 * that is no power of two in 16 .. 1024, min_cell > max_cell, texel not positive and finite, a class table that is not
 * ascending from 0 to the count or describes more than 16384 x 16384 texels, an atlas side outside 1 .. 16384 or no
 * multiple of min_cell, ray_ld < 6, a kind or filter that does not exist, a colour outside [0, 1]), -3 for a NULL pointer
 * that must not be. */
int hn_tex_classify(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces, float texel,
                    int min_cell, int max_cell, int32_t* class_dev, int64_t* keys_dev, int32_t* err_dev, hnStream_t stream);
int hn_tex_layout(const int64_t* sorted_keys_dev, long long n_faces, const int64_t* class_rank_host, int min_cell,
                  long long n_cells, int32_t* cell_start_dev, int32_t* cell_side_dev, int32_t* cell_face_dev, float* uv_dev,
                  hnStream_t stream);
int hn_tex_rasterize(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                     const float* normals_dev, const int32_t* cell_face_dev, long long n_cells,
                     const int64_t* class_cells_host, int min_cell, int H, int W, int32_t* owner_dev, float* position_dev,
                     float* normal_dev, hnStream_t stream);
int hn_tex_shade(const float* vertices_dev, long long n_vertices, const int32_t* faces_dev, long long n_faces,
                 const float* normals_dev, const float* uv_dev, const void* texture_dev, int texture_kind, int tex_h,
                 int tex_w, int filter, const float* rays_dev, int ray_ld, long long n_pixels, const int32_t* face_dev,
                 const float* bary_dev, int headlight, float ambient, const float* background_host, float* normal_out_dev,
                 float* rgb_out_dev, uint8_t* rgb8_out_dev, hnStream_t stream);

/* LPIPS v0.1 (csrc/hn_lpips.hip; DESIGN.md 3.14 holds the definition, tests/lpips_restated.py restates it in float64): the
 * layers of the frozen AlexNet / VGG16 backbones and the distance head, exact fp32, one entry point per layer kind; the
 * layer tables and the weights are the host's (ops/lpips/).  All tensors contiguous DEVICE fp32 unless said otherwise.
 *   hn_lpips_prepare    out (2n, 3, h, w): images [0, n) from pred, [n, 2n) from gt (each (n, 3, h, w) with arbitrary
 *                element strides, `*_strides`: HOST arrays of 4), every value ((2 v - 1) - shift_c) / scale_c with shift =
 *                (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450).  net: 0 AlexNet (sides >= 31), 1 VGG16 (>= 16).
 *   hn_lpips_conv       y (imgs, cout, oh, ow) = [relu](conv(x (imgs, cin, h, w)) + bias), square kernel 1 .. 15, zero
 *                padding pad < kernel, o = (side + 2 pad - kernel) / stride + 1 (floor).  An implicit GEMM on
 *                v_mfma_f32_32x32x2_f32: every output is one fmaf chain from 0 over k = (ci * kernel + ky) * kernel + kx
 *                ascending, then + bias: the same bits for every tile shape, batch size and run.  wt: the weights
 *                transposed and zero-padded, [Kpad][Mpad] with Kpad = K rounded up to 64, Mpad = cout rounded up to 128;
 *                ktab: Kpad int32, ci << 8 | ky << 4 | kx of row k, -1 for a padding row.  tile: 0 picks the tile shape
 *                (the largest of 128 x 128, 64 x 64, 32 x 64 (channels x pixels) whose grid has 256 workgroups), 1 / 2 / 3
 *                force one.
 *   hn_lpips_maxpool    y (planes, oh, ow) = max over kernel x kernel windows at stride `stride`, no padding, floor mode.
 *   hn_lpips_distance   feat (2n, c, h, w), the two images of pair i at i and n + i; lin (c) weights;
 *                out[i * 5 + layer] = mean over pixels of sum_c lin[c] * (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2,
 *                |.| the root of the sum of squares over channels.  One workgroup and one partial sum per 64
 *                pixels of a pair into `workspace` (hn_lpips_workspace_bytes: host arithmetic), a second launch adds a
 *                pair's partial sums in a fixed order: no float atomics, bit-reproducible.  out: (n, 5), other columns
 *                untouched.
 * Status, before any launch: -2 for every refused argument (a NULL pointer, a size <= 0, a side below the net's minimum,
 * a kernel above 15, more than 4096 channels, a tensor of more than 2^31 - 1 elements, n > 65535 pairs). */
int hn_lpips_prepare(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int n,
                     int h, int w, int net, float* out_dev, hnStream_t stream);
int hn_lpips_conv(const float* x_dev, const float* wt_dev, const float* bias_dev, const int32_t* ktab_dev, float* y_dev,
                  int imgs, int cin, int h, int w, int cout, int kernel, int stride, int pad, int relu, int tile,
                  hnStream_t stream);
int hn_lpips_maxpool(const float* x_dev, float* y_dev, int planes, int h, int w, int kernel, int stride, hnStream_t stream);
int hn_lpips_workspace_bytes(int n, int h, int w, int64_t* bytes);
int hn_lpips_distance(const float* feat_dev, const float* lin_dev, int n, int c, int h, int w, int layer, float* out_dev,
                      void* workspace, hnStream_t stream);

/* Background regularization (HyperNeRF's training loop; csrc/hn_regularizers.hip): static background points of the
 * capture go through the warp field under random warp embeddings and a robust loss pulls warp(p) back to p.
 *
 * hn_bg_sample draws the batch: with i = min(int(u[n][0] * m), m - 1) and j = min(int(u[n][1] * k), k - 1),
 *   out_points[n] = points[i] + noise_std * nrm[n]   (fp32; the product u * m in fp32, every multiply and add rounded on
 *                                                      its own: a float32 restatement is bit-exact)
 *   out_ids[n]    = ids[j]                           (int64)
 * points (m, 3) fp32, ids (k,) int64, u (n, 2) uniforms in [0, 1) and nrm (n, 3) normals as hn_random_fill writes them
 * (the sampler has no generator of its own).  The indices are clamped to their tables whatever u holds.  m and k at
 * most 2^24 (a 24-bit uniform reaches no further).
 *
 * hn_bg_loss_*: warped, points (n, 3) contiguous fp32; x_n = |warped_n - points_n|^2 / scale^2;
 *   loss = mean_n 2 x_n / (x_n + 4)                  (Barron's general loss at alpha = -2, Geman-McClure)
 *   d_warped_n = g 16 (warped_n - points_n) / (scale^2 (x_n + 4)^2 n);  `points` carries no gradient.
 * A zero residual gives loss 0 and gradient 0.  loss_out: ONE device float, written by one workgroup that adds in a fixed
 * order (no float atomics: bit-reproducible).  hn_bg_loss_forward_grad also writes the d_warped hn_bg_loss_backward
 * would write for g = 1, bit for bit; hn_bg_loss_backward reads g from g_loss (ONE device float).
 *
 * Status: -2 for every refused argument (a NULL pointer, n, m, k <= 0, m or k above 2^24, scale <= 0), checked on the
 * host before any launch. */
int hn_bg_sample(const float* points, int m, const int64_t* ids, int k, const float* u, const float* nrm, int n,
                 float noise_std, float* out_points, int64_t* out_ids, hnStream_t stream);
int hn_bg_loss_forward(const float* warped, const float* points, int n, float scale, float* loss_out, hnStream_t stream);
int hn_bg_loss_forward_grad(const float* warped, const float* points, int n, float scale, float* loss_out,
                            float* d_warped, hnStream_t stream);
int hn_bg_loss_backward(const float* warped, const float* points, int n, float scale, const float* g_loss,
                        float* d_warped, hnStream_t stream);

/* Distortion loss of Mip-NeRF 360 (Barron et al. 2022, eq. 15; csrc/hn_regularizers.hip) on ONE level's compositing
 * weights.  weights, z (n_rays, n_samples) contiguous fp32, both in the level's sorted order (z ascending along a ray),
 * n_samples <= 512.  Normalised distance
 *   s_i = (z_i - near) / (far - near)                  spacing 0 (linear)
 *   s_i = (1/z_i - 1/near) / (1/far - 1/near)          spacing 1 (disparity; near > 0)
 * Sample i < S-1 owns [s_i, s_{i+1}]: width d_i = s_{i+1} - s_i, midpoint m_i = (s_i + s_{i+1}) / 2; the last sample (the
 * compositing kernel's "infinite" interval) is a point mass: d = 0, m = s_{S-1}.
 *   L_ray = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i        loss = mean over rays of L_ray
 *   dL_ray/dw_i = 2 sum_j w_j |m_i - m_j| + (2/3) w_i d_i             (depths carry no gradient)
 * O(S) per ray (prefix and suffix sums; one wave per ray).  n_samples = 1 gives loss 0 and gradient 0.
 *
 * per_ray (n_rays) receives L_ray and is required: it is also what the mean is taken from.  loss_out: ONE device float,
 * the mean, added in a fixed order by the block that finishes last (no float atomics: bit-reproducible); NULL in
 * hn_distortion_forward = per-ray values only.  ticket: ONE device uint32 that is 0 before the first launch; the launch
 * leaves it 0 (needed whenever loss_out is given; launches that share a ticket must be stream-ordered).
 * hn_distortion_forward_grad also writes d_weights = grad_scale / n_rays * dL_ray/dw — bit for bit what
 * hn_distortion_backward writes for g_loss[0] == grad_scale.  hn_distortion_backward: g_loss is ONE device float (the
 * mean's incoming gradient) or, with per_ray_g != 0, n_rays floats (the incoming gradient of per_ray; no 1 / n_rays).
 *
 * Status: -2 for every refused argument (a NULL pointer, n_rays <= 0, n_samples <= 0 or > 512, far == near, a spacing
 * that is neither of the two, near <= 0 under disparity spacing, a NaN grad_scale), checked on the host before any launch. */
int hn_distortion_forward(const float* weights, const float* z, int n_rays, int n_samples, float near, float far,
                          int spacing, float* per_ray, float* loss_out, uint32_t* ticket, hnStream_t stream);
int hn_distortion_forward_grad(const float* weights, const float* z, int n_rays, int n_samples, float near, float far,
                               int spacing, float grad_scale, float* per_ray, float* loss_out, uint32_t* ticket,
                               float* d_weights, hnStream_t stream);
int hn_distortion_backward(const float* weights, const float* z, int n_rays, int n_samples, float near, float far,
                           int spacing, const float* g_loss, int per_ray_g, float* d_weights, hnStream_t stream);

/* torch.optim.Adam (the reference's default optimizer, utils/__init__.py get_optimizer) over ONE flat fp32 buffer
 * (ParamArena): p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps), m,v updated first, L2 weight decay added to the
 * gradient.  `hyper_dev`: 8 floats ON THE DEVICE, [lr, beta1, beta2, eps, weight_decay, grad_scale, 0, 0] — read by the
 * kernel, so a launch captured in a HIP graph follows a learning-rate schedule (utils/__init__.py:43-46) without
 * re-capture; grad_scale multiplies the gradient first (1/world after a SUM all-reduce).  `step_dev`: TWO 4-byte words
 * on the device, [0] = number of updates done so far as a float (advanced by the launch itself: the last block to
 * finish stores it), [1] = a ticket counter the launch leaves at zero.
 * zero_grad != 0 clears `grads` in the same pass.  Buffers 16-byte aligned. */
int hn_adam_step(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, long long n,
                 const float* hyper_dev, float* step_dev, int zero_grad, hnStream_t stream);

/* The other optimizers of the reference's get_optimizer (utils/__init__.py:23-41) over ONE flat fp32 buffer, launched
 * like hn_adam_step: `step_dev` = the same two words ([0] updates done as a float, advanced by the launch; [1] a ticket
 * the launch leaves at zero), zero_grad != 0 clears `grads`, grad_scale multiplies the gradient first.  The
 * hyper-parameters are DOUBLES on the device: the kernels compute the reference's schedule scalars (beta^t, N_sma, the
 * step size and its product with lr, Python doubles there) in fp64 once per workgroup and round each to fp32 once.
 * Status: -2 n <= 0 (or k < 1), -3 a NULL pointer that must not be, -4 a buffer not 16-byte aligned (hyper: 8).
 *
 * hn_sgd_step: torch.optim.SGD.  hyper_dev: 8 doubles [lr, momentum, dampening, weight_decay, nesterov (0/1),
 * grad_scale, 0, 0].  d = g*grad_scale + wd*p; with momentum != 0 (and momentum_buf != NULL) buf = d on update 1,
 * buf = momentum*buf + (1-dampening)*d after that, d = d + momentum*buf (Nesterov) or buf; p -= lr*d.  momentum_buf
 * may be NULL when momentum is 0. */
int hn_sgd_step(float* params_dev, float* grads_dev, float* momentum_buf_dev, long long n, const double* hyper_dev,
                float* step_dev, int zero_grad, hnStream_t stream);
/* hn_radam_step: RAdam (utils/optimizers.py:29-95) when slow_dev == NULL, Ranger (utils/optimizers.py:322-405, RAdam
 * with threshold N_sma > N_sma_threshhold, weight decay on every step and lookahead: slow = p before update 1, and after
 * every update t with t % k == 0 slow += alpha*(p - slow), p = slow) otherwise.  hyper_dev: 12 doubles [lr, beta1,
 * beta2, eps, weight_decay, grad_scale, N_sma_threshhold (Ranger), degenerated_to_sgd (RAdam, 0/1), alpha (Ranger), 0,
 * 0, 0].  k: Ranger's lookahead period (>= 1; RAdam ignores it, pass 1). */
int hn_radam_step(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* slow_dev,
                  long long n, int k, const double* hyper_dev, float* step_dev, int zero_grad, hnStream_t stream);

/* Gradient clipping over ONE flat fp32 gradient buffer (ParamArena.grad), ahead of a *_step launch:
 * torch.nn.utils.clip_grad_value_ and then torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite False) of the
 * gradient that counts, s * g with s = grad_scale > 0 (1 / world after a SUM all-reduce; the step launches apply s
 * themselves later).  clamp(s*g, +-v) = s * clamp(g, +-v/s), so both launches work on the raw buffer with the
 * threshold v' = fp32(clip_value / grad_scale), the division in double:
 *   total_norm = s * sqrt(sum clamp(g, +-v')^2)       coef = min(max_norm / (total_norm + 1e-6), 1)  (a NaN stays NaN)
 *   grad <- clamp(g, +-v') * coef                     (the clamp by comparisons: a NaN gradient stays NaN)
 * +inf for clip_value or max_norm means "off".
 *
 * hn_grad_norm: one launch on the step kernels' grid (at most 256 blocks x 256 threads).  fp32 sums of squares per
 * thread, wave and block in a fixed order, one partial per block in work[block]; the block that arrives last adds the
 * partials in index order in fp64 and writes out[0] = total_norm, out[1] = coef.  No float atomics: the same input
 * gives the same bits on every run and every graph replay.  `work`: 256 floats + 1 ticket word, 16-byte aligned, zeroed
 * ONCE by its owner (the launch leaves the ticket at zero).  `out`: 2 floats.  `grad` is only read.
 * hn_grad_scale: the same grid; every thread reads out[1] and the launch returns without touching `grad` when
 * coef == 1 and clip_value is +inf; otherwise one in-place pass.  out == NULL: value clipping only (coef 1).
 *
 * Status, checked before any launch: -2 n <= 0, or grad_scale / clip_value / max_norm not positive (NaN included);
 * -3 a NULL pointer that must not be; -4 grad or work not 16-byte aligned, out not 4-byte aligned. */
int hn_grad_norm(const float* grad_dev, long long n, float grad_scale, float clip_value, float max_norm,
                 float* work_dev, float* out_dev, hnStream_t stream);
int hn_grad_scale(float* grad_dev, long long n, float grad_scale, float clip_value, const float* out_dev,
                  hnStream_t stream);

/* All rays of one H x W image on the device: get_ray_directions + get_rays (+ get_ndc_rays when `ndc`)
 * (datasets/ray_utils.py:5-93) and the ray-row layout of datasets/llff.py:244-264:
 * rays[(j*W + i)] = [origin(3), direction(3), near, far(, image_id)], row_floats = 8 or 9.
 * c2w: (3,4) row-major fp32 on the device.  `ndc_near` is get_ndc_rays' near plane (the reference passes 1.0). */
int hn_generate_rays(int H, int W, float focal, const float* c2w_dev, int ndc, float ndc_near, float near,
                     float far, float image_id, int row_floats, float* rays_dev, hnStream_t stream);

/* One training batch of an LLFF dataset (datasets/llff.py's all_rays / all_rgbs, as a shuffled DataLoader reads them),
 * gathered on the device without a host round trip.  The dataset is n_rays = n_images*H*W rays: ray g is pixel
 * g % (H*W) of training slot g / (H*W).  For row r < batch: g = perm[state[0] + r];
 * rays[r] = the row hn_generate_rays writes for that pixel with c2w_dev[slot] ((n_images, 3, 4) fp32) and, for
 * row_floats 9, image_ids_dev[slot] (fp32); rgbs[r] = rgb8_dev[g] / 255 ((n_rays, 3) uint8; ToTensor's rounded
 * division).  state_dev: three uint64 words [cursor, arrival counter, error flag], zero-initialised by the caller;
 * the launch advances the cursor by `batch` and leaves the counter at 0.  A position at or past n_perm, or an index g
 * outside [0, n_rays), writes NaN into that row of rays and rgbs and sets the error flag to 1.  Graph-capturable. */
int hn_ray_batch(const int64_t* perm_dev, long long n_perm, unsigned long long* state_dev, int batch, long long n_rays,
                 int H, int W, float focal, const float* c2w_dev, const float* image_ids_dev, int ndc, float ndc_near,
                 float near, float far, int row_floats, const uint8_t* rgb8_dev, float* rays_dev, float* rgbs_dev,
                 hnStream_t stream);

/* hn_ray_batch over a Blender dataset (datasets/blender.py): rgba8_dev is (n_rays, 4) uint8 RGBA, 4-byte aligned, each
 * pixel read as one 32-bit word, and rgbs[r] is that pixel blended onto white exactly as hn_blend_white_u8 writes it
 * (one device function).  Everything else — state words, NaN rows and the error flag, the ray row — as hn_ray_batch. */
int hn_ray_batch_rgba(const int64_t* perm_dev, long long n_perm, unsigned long long* state_dev, int batch,
                      long long n_rays, int H, int W, float focal, const float* c2w_dev, const float* image_ids_dev,
                      int ndc, float ndc_near, float near, float far, int row_floats, const uint8_t* rgba8_dev,
                      float* rays_dev, float* rgbs_dev, hnStream_t stream);

/* All rays of one H x W image of a Nerfies-format capture (datasets/nerfies.py), rows as hn_generate_rays writes them.
 * cam_dev: that image's camera record of 24 fp32 on the device: orientation (9: world to camera, row-major),
 * position (3), focal_length, pixel_aspect_ratio, skew, principal point (cx, cy), radial distortion (k1, k2, k3),
 * tangential distortion (p1, p2), two zeros.  Pixel (col i, row j), centre (i + 0.5, j + 0.5):
 *   y = (j + 0.5 - cy) / (f*aspect);  x = (i + 0.5 - cx - y*skew) / f;  (x, y) <- undistort(x, y);
 *   direction = normalise(orientation^T normalise((x, y, 1)));  origin = position.
 * undistort: exactly 10 Newton steps from the distorted point on  D x + 2 p1 x y + p2 (r + 2 x^2) = xd,
 * D y + 2 p2 x y + p1 (r + 2 y^2) = yd,  r = x^2 + y^2,  D = 1 + r (k1 + r (k2 + k3 r)); a step whose determinant is
 * within 1e-9 of zero moves nothing; skipped when all five coefficients are zero.  No NDC. */
#define HN_NERFIES_CAM_FLOATS 24
int hn_generate_rays_nerfies(int H, int W, const float* cam_dev, float near, float far, float image_id, int row_floats,
                             float* rays_dev, hnStream_t stream);

/* hn_ray_batch over a Nerfies-format capture: cams_dev is the (n_images, 24) fp32 table of the camera records above,
 * rgb8_dev (n_rays, 3) uint8, and rays[r] is the row hn_generate_rays_nerfies writes for that pixel with cams_dev[slot]
 * (one device function) and, for row_floats 9, image_ids_dev[slot].  Everything else — state words, NaN rows and the
 * error flag, rgbs = u8 / 255 — as hn_ray_batch. */
int hn_ray_batch_nerfies(const int64_t* perm_dev, long long n_perm, unsigned long long* state_dev, int batch,
                         long long n_rays, int H, int W, const float* cams_dev, const float* image_ids_dev, float near,
                         float far, int row_floats, const uint8_t* rgb8_dev, float* rays_dev, float* rgbs_dev,
                         hnStream_t stream);

/* The reference's blend of an RGBA image onto white (datasets/blender.py:58, :93-95) on ToTensor values:
 * rgbs[i][k] = fl(fl(fl(c_k / 255) * al) + fl(1 - al)), al = fl(a / 255) — every operation rounded on its own, no fused
 * multiply-add — and, when mask_dev != NULL, mask[i] = (a > 0) as one byte.  rgba8_dev: (n, 4) uint8, 4-byte aligned;
 * rgbs_dev: (n, 3) fp32. */
int hn_blend_white_u8(const uint8_t* rgba8_dev, long long n, float* rgbs_dev, uint8_t* mask_dev, hnStream_t stream);

/* Pillow's conversions around a resize of an RGBA image (n pixels, 4-byte aligned; in_dev == out_dev allowed).
 * inverse = 0, RGBA -> premultiplied: c' = ((t >> 8) + t) >> 8 with t = c*a + 128.  inverse = 1, back: the bytes stay
 * for a == 0 or a == 255, else c = min(255, (255*c') / a) in integer division.  Alpha is copied. */
int hn_premultiply_u8(const uint8_t* in_dev, long long n, int inverse, uint8_t* out_dev, hnStream_t stream);

/* One pass of Pillow's 8-bit Image.resize (ImagingResampleHorizontal_8bpc / Vertical_8bpc), bit-exact given its
 * tables: out = clamp(((1 << 21) + sum_k in[bounds[2o] + k] * kk[o*ksize + k]) >> 22, 0, 255) per channel, k <
 * bounds[2o+1].  in: (rows, cols, channels) uint8; vertical = 0 resamples along cols into (rows, out_len, channels),
 * vertical = 1 along rows into (out_len, cols, channels).  bounds (out_len, 2) [first, count] and kk (out_len, ksize)
 * int32 (22 fraction bits) on the device; the caller keeps first + count within the input axis. */
int hn_resample_u8(const uint8_t* in_dev, int rows, int cols, int channels, int out_len, int vertical,
                   const int32_t* bounds_dev, const int32_t* kk_dev, int ksize, uint8_t* out_dev, hnStream_t stream);

/* SE(3) exponential-map warp of warping.SE3Field.warp (hypernerf/warping.py:226-238 with rigid_body.exp_se3,
 * rigid_body.py:55-83, applied per point): theta = |w|, a = w/theta, b = v/theta,
 * y = p + sin(theta) a x p + (1-cos(theta)) a x (a x p) + theta b + (1-cos(theta)) a x b + (theta-sin(theta)) a x (a x b),
 * evaluated without the division by theta (smooth coefficients of w x ., w x (w x .)): accurate to a few fp32 units at
 * every theta, and theta = 0 is the pure translation y = p + v with finite gradients (d w = p x g + (v x g)/2).
 * w, v, points, out: (n_points, 3) fp32 row-major.  The backward writes the gradients w.r.t. w, v and points
 * (each may be NULL). */
int hn_se3_apply_forward(const float* w, const float* v, const float* points, int n_points, float* out,
                         hnStream_t stream);
int hn_se3_apply_backward(const float* w, const float* v, const float* points, const float* g_out, int n_points,
                          float* d_w, float* d_v, float* d_points, hnStream_t stream);

/* The same warp with a row stride per operand (w and v = the two halves of the field's (P, 6) head output, g_out =
 * columns of the template's source-gradient tensor: no slicing copies on either side), and — forward — an optional
 * second output rows_out (P, 3 + H), row stride rows_ld = [y | table[idx[p / samples_per_ray]]]: the `warped_points`
 * tensor of an axis-aligned-plane level (hypernerf/models.py:533-534, 578-581) without index_select + cat; an index
 * outside [0, n_rows) writes NaN, as the machine's own gather does.  out (P, 3) contiguous may be NULL if rows_out is
 * given; d_w / d_v / d_points may each be NULL. */
int hn_se3_warp_forward(const float* w, int w_ld, const float* v, int v_ld, const float* points, int p_ld,
                        int n_points, float* out, float* rows_out, int rows_ld, const float* table,
                        const int64_t* idx, int H, int n_rows, int samples_per_ray, hnStream_t stream);
int hn_se3_warp_backward(const float* w, int w_ld, const float* v, int v_ld, const float* points, int p_ld,
                         const float* g_out, int g_ld, int n_points, float* d_w, int dw_ld, float* d_v, int dv_ld,
                         float* d_points, hnStream_t stream);

/* The GIF of the evaluated frames (eval.py:172, imageio.mimsave) and the depth image of the validation step
 * (utils/visualization.py:6-18): csrc/hn_gif.hip.  Pixels are packed 8-bit RGB, (n, 3) uint8 with NO alignment assumed;
 * 1 <= n <= 2^31 everywhere.  Status, checked before any launch and before anything is written: -2 a count out of range,
 * -3 a NULL pointer, -4 a misaligned word buffer (hist: 8 bytes; depth, range: 4 bytes).
 *
 * hn_color_hist: hist (2^18, 4) uint64, cell key = (r>>2)<<12 | (g>>2)<<6 | b>>2, holds [pixels, sum r, sum g, sum b].
 * The launch ADDS to the table (the caller zeroes it; several frames may feed one table).  64-bit integer adds: exact for
 * any number of calls that stays below 2^64 / 255 pixels per cell, and independent of arrival order.  Equal keys are
 * folded per wave and, for the key of a workgroup's first pixel, per workgroup, before one add reaches memory.
 * hn_palette_map: index[i] = argmin over k < n_colors (1..256) of (r-pr)^2 + (g-pg)^2 + (b-pb)^2 in integers against
 * palette (n_colors, 3) uint8, the smallest k among equal distances; index (n,) uint8. */
#define HN_HIST_BINS 262144 /* 2^18 cells of hn_color_hist's table, one per colour key */
int hn_color_hist(const uint8_t* rgb_dev, long long n, unsigned long long* hist_dev, hnStream_t stream);
int hn_palette_map(const uint8_t* rgb_dev, long long n, const uint8_t* palette_dev, int n_colors, uint8_t* index_dev,
                   hnStream_t stream);

/* visualize_depth in two launches without a host read between them.  d = nan_to_num(depth): NaN -> 0, +-inf -> +-FLT_MAX.
 * hn_depth_range: range[0] = min d, range[1] = max d (one workgroup: depth maps are image-sized; the sign of a zero
 * minimum or maximum is unspecified, and changes no pixel).
 * hn_depth_colormap: x = (d - range[0]) / (range[1] - range[0] + 1e-8f), every operation rounded on its own in fp32;
 * k = (uint8)(255 * x) by truncation; out[i] = lut[k] for a (256, 3) uint8 table; out (n, 3) uint8.  Where x is NaN
 * (range[1] - range[0] overflowed) k = 0: NumPy's cast is undefined there, this is the one stated deviation. */
int hn_depth_range(const float* depth_dev, long long n, float* range_dev, hnStream_t stream);
int hn_depth_colormap(const float* depth_dev, long long n, const float* range_dev, const uint8_t* lut_dev,
                      uint8_t* out_dev, hnStream_t stream);

/* GIF's variable-width LZW of n >= 0 palette indices with minimum code size 8.  HOST code, host pointers, no launch and
 * no stream: the chain of codes is serial and the frame is on its way to a file.  The clear code 256 comes first; codes
 * are 9 to 12 bits, packed least significant bit first; when the 4096 codes are used up a clear code is sent and the
 * table starts over; the end code 257 closes the stream.  out receives the raw code bytes (the caller cuts them into
 * sub-blocks of at most 255) and *out_len their number.  -2: n or capacity negative; -3: a NULL pointer that must not be;
 * -6: the stream needs *out_len bytes and `capacity` is smaller (nothing is written past capacity). */
int hn_gif_lzw(const uint8_t* indices, long long n, uint8_t* out, long long capacity, long long* out_len);

/* Box calibration for a benchmark line (no reference counterpart: measurement infrastructure).  Both kernels time
 * themselves into t_dev (device uint64[16], zeroed by the caller; layout of HnMlpArgs.timeline in [0..7]).
 * hn_calib_mfma: every wave of 512 workgroups x 8 waves runs `iters` x 8 independent v_mfma_f32_32x32x16_bf16 from
 * registers — FLOPs = 512 * 8 * iters * 8 * 32768; t[8] / t[9] = shader-clock (s_memtime) / 100 MHz wall-clock ticks of
 * one wave's loop, i.e. the sustained shader clock = 1e8 * t[8] / t[9] Hz.
 * hn_calib_stream: 256 workgroups stream n_bytes (a multiple of 64 KiB is read) once through LDS-DMA. */
int hn_calib_mfma(int iters, float* sink_dev, uint64_t* t_dev, hnStream_t stream);
int hn_calib_stream(const void* buf_dev, long long n_bytes, float* sink_dev, uint64_t* t_dev, hnStream_t stream);
/* pattern 0: as hn_calib_stream (the workgroups share one moving window); 1: every workgroup streams a contiguous region
 * of its own, front to back — 256 far-apart sequential streams, the pattern of hn_wgrad_kernel's jobs. */
int hn_calib_stream_pattern(const void* buf_dev, long long n_bytes, int pattern, float* sink_dev, uint64_t* t_dev,
                            hnStream_t stream);
/* The DMA protocol of hn_wgrad_kernel alone: a ring of `stages` (3, 4, 5) stages of 32 KiB, counted vmcnt wait for the
 * oldest stage, proto 0: + a workgroup barrier per stage (the kernel's), proto 1: no barrier. */
int hn_calib_ring(const void* buf_dev, long long n_bytes, int stages, int proto, float* sink_dev, uint64_t* t_dev,
                  hnStream_t stream);

/* Debug/probe: runs one MFMA of each kind on identifiable data (layout self-test on real hardware). */
int hn_probe_mfma(float* out_bf16_acc, float* out_f32_acc, float* out_glds, hnStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
