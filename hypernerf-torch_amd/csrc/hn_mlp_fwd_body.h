// Body of the forward machine kernels: the statements of hn_mlp_fwd_kernel and hn_mlp_fwd_relu_kernel (hn_mlp.hip), which
// include this file inside their function bodies.  In scope there: the kernel argument `const HnMlpArgs a` and the
// compile-time flags BF16, AUXG, EXTRA, TRAIN, S8, ACTS.  Not a stand-alone header.
  using M = ModeT<BF16>;
  constexpr int SX = S8 ? 1 : 0;
  static_assert(!(S8 && (EXTRA || !TRAIN || !BF16)), "the 8-bit stash exists for the render-level bf16 training builds only");
  if constexpr (S8) asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");     // FP16_OVFL: 8-bit conversions clamp
  using Frag = typename M::Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  constexpr int PTS = M::WAVES * 32;
  const int ntiles = (a.n_points + PTS - 1) / PTS;
  hn_timeline_begin(a.timeline);
#ifdef HN_PROF
  long long* prof_buf = reinterpret_cast<long long*>(a.prof);
  const bool prof_on = prof_buf != nullptr && blockIdx.x == 0 && wave == 0;
  int prof_n = 0;
#endif

  WStream<M::WAVES> ws;
  ws.g = reinterpret_cast<const char*>(a.wstream);
  ws.lds = smem;
  ws.nchunks = a.n_chunks;
  ws.wave = wave;
  ws.lane = lane;

  Frag cur[8 * M::STEPS32];
  Frag nxt[8 * M::STEPS32];

  // biases and the feature table live in LDS for the whole kernel: no global loads inside the MFMA loops
  float* bias_lds = reinterpret_cast<float*>(smem + 2 * HN_CHUNK_UNITS * 1024);
  HnFeat* feat_lds = reinterpret_cast<HnFeat*>(bias_lds + ((a.n_bias + 3) & ~3));
  HnDFeat* dfeat_lds = reinterpret_cast<HnDFeat*>(feat_lds + ((a.n_feat + 1) & ~1));      // bf16 kernels only
  // per wave: value plane (n_comps x 32 floats) and, bf16 only, the (hi, lo) planes of x / 2pi for the first n_trig
  const int n_trig = BF16 ? a.n_trig_comps : 0;
  const bool with_lo = a.trig_lo_planes != 0;
  const int n_planes = BF16 ? a.n_comps + n_trig + (with_lo ? n_trig : 1) : a.n_comps;
  float* srcv = reinterpret_cast<float*>(BF16 ? reinterpret_cast<char*>(dfeat_lds + a.n_feat)
                                              : reinterpret_cast<char*>(dfeat_lds)) + wave * (n_planes * 32);
  float* rev = BF16 ? srcv + a.n_comps * 32 : nullptr;
  for (int i = threadIdx.x; i < a.n_bias; i += blockDim.x) bias_lds[i] = a.bias[i];
  for (int i = threadIdx.x; i < a.n_feat; i += blockDim.x) {
    const HnFeat e = a.feat[i];
    feat_lds[i] = e;
    if constexpr (BF16) dfeat_lds[i] = hn_derive_feat_fwd(e, a.n_comps, n_trig, with_lo);
  }
  __syncthreads();

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int blk = tile * M::WAVES + wave;  // 32-point block of this wave
    const int p0 = blk * 32 + r;
    const bool valid = p0 < a.n_points;
    const int p = valid ? p0 : a.n_points - 1;
    const int ray = p / a.samples_per_ray;
    const bool wave_valid = blk * 32 < a.n_points;  // wave-uniform: the block holds at least one point
    hn_stage_sources(srcv, a, p, ray, lane, rev, n_trig, with_lo);
    ws.start();

    HnOpWords w_next = hn_load_op(a.ops, 0, a.n_ops);
    for (int op = 0; op < a.n_ops; ++op) {
      const HnOpWords w = w_next;
      w_next = hn_load_op(a.ops, op + 1, a.n_ops);
      const int code = w[0];
      if (code == HN_OP_LAYER) {
        HN_STAMP(100 + op);
        const int K32 = w[1] & 255, nG = (w[1] >> 8) & 255, NT = (w[1] >> 16) & 255;
        const int act = (w[1] >> 24) & 15, flags = (w[1] >> 28) & 15;
        const float* bias = bias_lds + w[2];
        const bool do_mask = TRAIN && w[4] >= 0 && wave_valid && !(ACTS && act == HN_ACT_SOFTPLUS);   // (softplus: w4 = p1)
        const bool do_stash = TRAIN && w[5] >= 0 && wave_valid;
        char* out_base = do_stash ? hn_slot_base<BF16, SX>(a, w[5], NT, blk) : nullptr;
        char* aux_base = (TRAIN && wave_valid) ? hn_slot_base<BF16, SX>(a, w[6], 2 * nG, blk) : nullptr;
        uint32_t* mask_base = do_mask ? hn_mask_base(a, w[4], (NT + 1) >> 1, blk, lane) : nullptr;
        const bool has_out = w_next[0] == HN_OP_OUT;    // head layer: its <=4 outputs leave from the accumulator
        const HnOpWords out_w = w_next;
        Frag aux[AUXG * 2 * M::STEPS32];
#pragma unroll
        for (int g = 0; g < AUXG; ++g) {
          if (g < nG) {
            if (EXTRA && (flags & HN_LAYER_DIRECT))
              hn_make_group<true>(aux + g * 2 * M::STEPS32, feat_lds + w[3] + 64 * g, dfeat_lds + w[3] + 64 * g, srcv,
                                  lane, a, p, ray);
            else
              hn_make_group<false>(aux + g * 2 * M::STEPS32, feat_lds + w[3] + 64 * g, dfeat_lds + w[3] + 64 * g, srcv,
                                   lane, a, p, ray);
            if (aux_base != nullptr) {
              hn_stash<BF16, SX>(aux + g * 2 * M::STEPS32, aux_base, 2 * g, lane);
              hn_stash<BF16, SX>(aux + (g * 2 + 1) * M::STEPS32, aux_base, 2 * g + 1, lane);
            }
          }
        }
        unsigned bits = 0;
        HN_STAMP(1);
        if constexpr (BF16) {
          // plain 128 -> 128 ReLU layers (template rgb branch, warp field) take the pipelined body (adding the 64-wide
          // shape as well tips the register allocator into spilling inside the generic path: measured 7 % slower)
          const bool plain = nG == 0 && act == HN_ACT_RELU && !(flags & HN_LAYER_NO_COMMIT) && !has_out &&
                             wave_valid && do_stash == do_mask;
          if (plain && K32 == 4 && NT == 4) {
            if (do_stash) hn_layer_pipelined<4, 4, true, SX>(cur, nxt, bias, ws, out_base, mask_base, lane);
            else hn_layer_pipelined<4, 4, false, SX>(cur, nxt, bias, ws, out_base, mask_base, lane);
            continue;
          }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (t < NT) {
            f32x16 acc;
            hn_init_acc(acc, bias, t, h);
            hn_gemm_k<BF16>(acc, cur, K32, ws);
#pragma unroll
            for (int g = 0; g < AUXG; ++g)
              if (g < nG) hn_gemm_blocks<BF16, 2>(acc, aux + g * 2 * M::STEPS32, ws);
            HN_STAMP(2);
            if (act == HN_ACT_RELU) {
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                bits = hn_push_mask<BF16>(bits, acc[i]);
                acc[i] = __int_as_float(max(__float_as_int(acc[i]), 0));  // relu on the bit pattern: one v_max_i32
              }
            } else if (ACTS && act != HN_ACT_NONE) {
              hn_act_tile<BF16>(acc, act, __int_as_float(w[7]), __int_as_float(w[4]), bits);
            }
            if (has_out && t == 0 && h == 0 && valid) {
              // the OUT op that follows a head layer: <= 4 fp32 columns straight from the accumulator
              const HnDst d = a.dst[out_w[1]];
              const int n = out_w[3];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                if (i < n) {
                  float y = acc[i];
                  if (out_w[4] == 1) y = 1.0f / (1.0f + expf(-y));
                  if (out_w[5] >= 0) {
                    const HnSrc sr = a.src[out_w[5]];
                    y = __fadd_rn(sr.ptr[(size_t)(sr.per_ray ? ray : p) * sr.ld + out_w[6] + i], y);
                  }
                  d.ptr[(size_t)p * d.ld + out_w[2] + i] = y;
                }
              }
            }
            if (has_out && t == 0 && h == 0 && out_w[7] > 0) {
              // publish the head's results as staged components of this block (every lane: padded points too)
              const int n = out_w[3];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                if (i < n) {
                  float y = acc[i];
                  if (out_w[4] == 1) y = 1.0f / (1.0f + expf(-y));
                  if (out_w[5] >= 0) {
                    const HnSrc sr = a.src[out_w[5]];
                    y = __fadd_rn(sr.ptr[(size_t)(sr.per_ray ? ray : p) * sr.ld + out_w[6] + i], y);
                  }
                  const int ci = out_w[7] - 1 + i;
                  srcv[ci * 32 + r] = y;
                  if (BF16 && ci < n_trig) {
                    float hi, lo;
                    hn_rev_split(y, hi, lo);
                    rev[ci * 32 + r] = hi;
                    if (with_lo) rev[(n_trig + ci) * 32 + r] = lo;
                  }
                }
              }
            }
            hn_acc_to_frags(acc, nxt + t * M::STEPS32);
#ifdef HN_PROF
            if (prof_on) {   // make the stamp wait for the tile's results
              float x__ = acc[15];
              asm volatile("v_mov_b32 %0, %0" : "+v"(x__)::"memory");
            }
#endif
            HN_STAMP(3);
            if ((t & 1) || t == NT - 1) {
              // a plain (cached) store: the backward machine stalls on these words at the top of every layer, and
              // unlike the once-streamed stash they are small enough (70 MB per step) to survive in L2 / MALL
              if (do_mask) mask_base[(t >> 1) * 64 + lane] = (t & 1) ? bits : bits << 16;
              bits = 0;
            }
            if (do_stash) {
              if constexpr (SX != 0) hn_stash8_acc<SX>(acc, out_base, t, lane);
              else hn_stash<BF16, SX>(nxt + t * M::STEPS32, out_base, t, lane);
            }
            HN_STAMP(4);
          }
        }
        if (!(flags & HN_LAYER_NO_COMMIT)) {
#pragma unroll
          for (int t = 0; t < 8; ++t)
            if (t < NT)
#pragma unroll
              for (int s = 0; s < M::STEPS32; ++s) cur[t * M::STEPS32 + s] = nxt[t * M::STEPS32 + s];
        }
      } else if (code == HN_OP_OUT) {
        // handled inside the LAYER op it follows (the raw accumulator is only alive there)
      } else if (EXTRA && code == HN_OP_OUT_WIDE) {
        const int n = w[3], NT = w[4];
        if (valid) {
          const HnDst d = a.dst[w[1]];
#pragma unroll
          for (int t = 0; t < 8; ++t)
            if (t < NT) {
              if constexpr (BF16) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                  for (int j = 0; j < 8; ++j) {
                    const int row = 32 * t + 16 * s + hn_pi16(h, j);
                    if (row < n) d.ptr[(size_t)p * d.ld + w[2] + row] = (float)cur[2 * t + s][j];
                  }
              } else {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                  const int row = 32 * t + hn_rho(q, h);
                  if (row < n) d.ptr[(size_t)p * d.ld + w[2] + row] = cur[16 * t + q];
                }
              }
            }
        }
      }
    }
  }
  hn_timeline_end(a.timeline);
