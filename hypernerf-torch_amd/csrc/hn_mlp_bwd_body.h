// Body of the backward-data machine kernels: the statements of hn_mlp_bwd_kernel and hn_mlp_bwd_relu_kernel (hn_mlp.hip),
// which include this file inside their function bodies.  In scope there: the kernel argument `const HnMlpArgs a` and
// the compile-time flags BF16, WIDE, S8, ACTS.  Not a stand-alone header.
  using M = ModeT<BF16>;
  constexpr int SZ = S8 ? 2 : 0;
  static_assert(!(S8 && WIDE) && !(S8 && !BF16), "the 8-bit stash exists for the render-level bf16 builds only");
  if constexpr (S8) asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");     // FP16_OVFL: 8-bit conversions clamp
  const float dz_scale = S8 ? ldexpf(1.0f, a.dz_scale_log2) : 1.0f;
  const float dz_unscale = S8 ? ldexpf(1.0f, -a.dz_scale_log2) : 1.0f;
  using Frag = typename M::Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  constexpr int PTS = M::WAVES * 32;
  const int ntiles = (a.n_points + PTS - 1) / PTS;
  HnFeat* feat_lds = reinterpret_cast<HnFeat*>(smem + 2 * HN_CHUNK_UNITS * 1024);
  HnDFeat* dfeat_lds = reinterpret_cast<HnDFeat*>(feat_lds + ((a.n_feat + 1) & ~1));      // bf16 kernel only
  float* srcv = reinterpret_cast<float*>(BF16 ? reinterpret_cast<char*>(dfeat_lds + a.n_feat)
                                              : reinterpret_cast<char*>(dfeat_lds)) + wave * (a.n_comps * 32);
  hn_timeline_begin(a.timeline);
#ifdef HN_PROF
  long long* prof_buf = reinterpret_cast<long long*>(a.prof);
  const bool prof_on = prof_buf != nullptr && blockIdx.x == 0 && wave == 0;
  int prof_n = 0;
#endif
  for (int i = threadIdx.x; i < a.n_feat; i += blockDim.x) {
    const HnFeat e = a.feat[i];
    feat_lds[i] = e;
    if constexpr (BF16) dfeat_lds[i] = hn_derive_feat(e);
  }
  __syncthreads();

  WStream<M::WAVES> ws;
  ws.g = reinterpret_cast<const char*>(a.wstream);
  ws.lds = smem;
  ws.nchunks = a.n_chunks;
  ws.wave = wave;
  ws.lane = lane;

  Frag cur[8 * M::STEPS32];
  Frag nxt[8 * M::STEPS32];
  Frag cur2[M::STEPS32];

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int blk = tile * M::WAVES + wave;
    const int p0 = blk * 32 + r;
    const bool valid = p0 < a.n_points;
    const int p = valid ? p0 : a.n_points - 1;
    const int ray = p / a.samples_per_ray;
    const bool wave_valid = blk * 32 < a.n_points;
    f32x16 dacc;  // source gradients of the block: row rho(i,h) = dsrc column, col r = point
    hn_init_acc(dacc, nullptr, 0, h);
    hn_stage_sources(srcv, a, p, ray, lane);
    ws.start();

    HnOpWords w_next = hn_load_op(a.ops, 0, a.n_ops);
    unsigned mnext[4] = {0u, 0u, 0u, 0u};
    bool mnext_ready = false;
    for (int op = 0; op < a.n_ops; ++op) {
      const HnOpWords w = w_next;
      w_next = hn_load_op(a.ops, op + 1, a.n_ops);
      const int code = w[0];
      HN_STAMP(100 * code + op);
      if (code != HN_BOP_LAYER && code != HN_BOP_AUX) mnext_ready = false;   // LOAD ops do not prefetch
      if (code == HN_BOP_LOAD) {
        // dZ (<= 4 columns) of an output layer -> one 32-feature tile
        const int n = w[3] & 255;
        const bool to2 = (w[3] >> 8) & 1;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if ((w[3] >> 9) & 1) {
          // the gradient later ops left in the source-gradient accumulators for the components this head published:
          // slots 8q + i sit in registers 4q + i of the h == 0 lanes (row rho(4q + i, 0) = 8q + i)
          const int q = (w[3] >> 10) & 3;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            d[i] = q == 0 ? dacc[i] : (q == 1 ? dacc[4 + i] : (q == 2 ? dacc[8 + i] : dacc[12 + i]));
        }
        if (h == 0 && valid) {
          const HnSrc s = a.src[w[1] < 0 ? 0 : w[1]];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i < n) {
              float g = (w[1] >= 0 && s.ptr != nullptr) ? s.ptr[(size_t)p * s.ld + w[2] + i] : 0.0f;
              if constexpr (S8) g *= dz_scale;
              if ((w[3] >> 9) & 1) g += d[i];
              if (w[4] == 1) {
                const HnSrc ys = a.src[w[5]];
                const float y = ys.ptr[(size_t)p * ys.ld + w[6] + i];
                g = g * y * (1.0f - y);
              }
              d[i] = g;
            } else {
              d[i] = 0.0f;
            }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) d[i] = 0.0f;
        }
        Frag tmp[M::STEPS32];
        hn_zero_frags(tmp, M::STEPS32);
        if constexpr (BF16) {
#pragma unroll
          for (int i = 0; i < 4; ++i) tmp[0][i] = (__bf16)d[i];  // h==0, j<4 <-> features 0..3
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) tmp[i] = d[i];             // step q, h==0 <-> feature q
        }
        if (a.training && w[7] >= 0 && wave_valid) hn_stash<BF16, SZ>(tmp, hn_slot_base<BF16, SZ>(a, w[7], 1, blk), 0, lane);
#pragma unroll
        for (int s = 0; s < M::STEPS32; ++s) {
          if (to2) cur2[s] = tmp[s];
          else cur[s] = tmp[s];
        }
      } else if (WIDE && code == HN_BOP_LOAD_WIDE) {
        const int n = w[3] & 0xffff, NT = w[4], dact = (w[3] >> 16) & 15;
        const HnSrc s = a.src[w[1]];
        unsigned nbits = 0xffffffffu;  // complement of the mask word: set = keep
        char* dz_base = (a.training && wave_valid) ? hn_slot_base<BF16>(a, w[7], NT, blk) : nullptr;
        const bool has_mask = w[5] >= 0 && dact != HN_ACT_SOFTPLUS;              // (softplus: w5 = p1)
        const bool from_y = (dact == HN_ACT_ELU || dact == HN_ACT_SOFTPLUS) && wave_valid;
        const char* y_base = from_y ? hn_slot_base<BF16>(a, w[7], NT, blk) : nullptr;  // y, stashed by the forward
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (t < NT) {
            if (has_mask && !(t & 1)) {  // output activation was relu / leaky relu: dZ = dY * f'(mask)
              nbits = wave_valid ? ~hn_mask_base(a, w[5], (NT + 1) >> 1, blk, lane)[(t >> 1) * 64 + lane] : 0u;
            }
            f32x16 v;
            if (dact == 0) {
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int row = 32 * t + hn_rho(i, h);
                const bool keep = hn_keep_mask(nbits, t & 1, i) != 0;
                v[i] = (valid && keep && row < n) ? s.ptr[(size_t)p * s.ld + w[2] + row] : 0.0f;
              }
            } else {
              const float p0 = __int_as_float(w[6]), p1 = __int_as_float(w[5]);
              f32x16 y = {0};
              if (y_base != nullptr) y = hn_unstash<BF16>(y_base, t, lane);
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int row = 32 * t + hn_rho(i, h);
                const float g = (valid && row < n) ? s.ptr[(size_t)p * s.ld + w[2] + row] : 0.0f;
                float d = 1.0f;
                if (dact == HN_ACT_LEAKY_RELU) d = hn_keep_mask(nbits, t & 1, i) != 0 ? 1.0f : p0;
                else d = hn_dact_y<BF16>(dact, y[i], p0, p1);
                v[i] = g * d;
              }
            }
            hn_acc_to_frags(v, cur + t * M::STEPS32);
            if (dz_base != nullptr) hn_stash<BF16>(cur + t * M::STEPS32, dz_base, t, lane);
          }
        }
      } else if (code == HN_BOP_LAYER) {
        const int K32 = w[1] & 255, K32b = (w[1] >> 8) & 255, NT = (w[1] >> 16) & 255;
        const bool has_mask = w[4] >= 0;
        const bool do_stash = a.training && w[5] >= 0 && wave_valid;
        char* dz_base = do_stash ? hn_slot_base<BF16, SZ>(a, w[5], NT, blk) : nullptr;
        const int dact = ACTS ? w[2] : 0;      // 0: relu' from the mask (or nothing); else HN_ACT_LEAKY_RELU / ELU / SOFTPLUS
        const char* y_base = (ACTS && !S8 && (dact == HN_ACT_ELU || dact == HN_ACT_SOFTPLUS) && wave_valid)
                                 ? hn_slot_base<BF16>(a, w[6], NT, blk) : nullptr;
        unsigned nbits = 0xffffffffu;
        unsigned mbits[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};  // complemented words: set = keep
        if (has_mask) {
          if (mnext_ready) {   // fetched while the previous op ran (hn_prefetch_masks): no memory wait here
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) mbits[dd] = ~mnext[dd];
          } else {             // all relu masks of the layer up front: one VMEM wait per layer, none per tile
            const uint32_t* mb = hn_mask_base(a, w[4], (NT + 1) >> 1, blk, lane);
#pragma unroll
            for (int dd = 0; dd < 4; ++dd)
              if (2 * dd < NT)
                mbits[dd] = wave_valid ? ~mb[dd * 64 + lane] : 0u;
          }
        }
        mnext_ready = false;
        if constexpr (BF16 && !ACTS && !WIDE && !S8 && HN_BWD_PIPE != 0) {
          // plain 128 -> 128 layers (warp field, template rgb branch): relu' from the mask, dZ stashed
          if (K32 == 4 && NT == 4 && K32b == 0 && has_mask && do_stash) {
            hn_bwd_layer_pipelined<4, 4>(cur, nxt, ws, mbits, dz_base, lane, a, w_next, blk, mnext, mnext_ready);
            continue;
          }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          if (t < NT) {
            f32x16 acc;
            hn_init_acc(acc, nullptr, t, h);
            hn_gemm_k<BF16>(acc, cur, K32, ws);
            if (K32b) hn_gemm_blocks<BF16, 1>(acc, cur2, ws);
            // the next layer's mask words, issued behind this tile's chunk barrier so that they have the rest of
            // the layer to arrive (the backward machine used to stall ~3 us on them at the top of every layer)
            if (t == 0) mnext_ready = hn_prefetch_masks(a, w_next, blk, lane, wave_valid, mnext);
            HN_STAMP(2);
            if (!(t & 1)) nbits = mbits[t >> 1];
            // dZ of padded points is zero from the LOAD ops on and stays zero: no `valid` select here
            if (dact == 0) {
#pragma unroll
              for (int i = 0; i < 16; ++i)
                acc[i] = __int_as_float(__float_as_int(acc[i]) & hn_keep_mask(nbits, t & 1, i));
            } else if (dact == HN_ACT_LEAKY_RELU) {
              const float p0 = __int_as_float(w[3]);
#pragma unroll
              for (int i = 0; i < 16; ++i)
                if (hn_keep_mask(nbits, t & 1, i) == 0) acc[i] *= p0;
            } else if (y_base != nullptr) {
              const f32x16 y = hn_unstash<BF16>(y_base, t, lane);
              const float p0 = __int_as_float(w[3]), p1 = __int_as_float(w[7]);
#pragma unroll
              for (int i = 0; i < 16; ++i) acc[i] *= hn_dact_y<BF16>(dact, y[i], p0, p1);
            }
            hn_acc_to_frags(acc, nxt + t * M::STEPS32);
            if (do_stash) {
              if constexpr (SZ != 0) hn_stash8_acc<SZ>(acc, dz_base, t, lane);
              else hn_stash<BF16, SZ>(nxt + t * M::STEPS32, dz_base, t, lane);
            }
            HN_STAMP(4);
          }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t)
          if (t < NT)
#pragma unroll
            for (int s = 0; s < M::STEPS32; ++s) cur[t * M::STEPS32 + s] = nxt[t * M::STEPS32 + s];
      } else if (code == HN_BOP_AUX) {
        // gradient of generated features: per 32-feature tile tmp = W_aux^T . dZ, then the chain rule
        const int K32 = w[1] & 255, K32b = (w[1] >> 8) & 255, nG = (w[1] >> 16) & 255;
        // w2: bit tt = tile tt holds a feature that differentiates into a source (the others are neither in the weight
        // stream nor computed: encoders of plain inputs in front of a GLO row, padding); bit 8 + tt = one of them is
        // trigonometric (a tile of identity features only — GLO rows — takes W^T dZ as it is: d feature / dx = 1)
        const int tiles = w[2];
        bool first = true;
        mnext_ready = false;
        for (int tt = 0; tt < 2 * nG; ++tt) {
          if (!((tiles >> tt) & 1)) continue;
          f32x16 acc;
          hn_init_acc(acc, nullptr, 0, h);
          hn_gemm_k<BF16>(acc, cur, K32, ws);
          if (K32b) hn_gemm_blocks<BF16, 1>(acc, cur2, ws);
          if (first) mnext_ready = hn_prefetch_masks(a, w_next, blk, lane, wave_valid, mnext);
          first = false;
          // chain rule per feature, then the reduction over the features of each source component as one more
          // matrix product: dacc[slot][point] += S[slot][feature] . G[feature][point]  (S: 0/1 selection block that
          // the host put in the weight stream right behind this tile's weights).  No LDS accumulators: an LDS
          // atomic after an LDS-DMA makes the compiler drain vmcnt, i.e. the weight prefetch.
          const HnFeat* ft = feat_lds + w[3] + 32 * tt;
          if ((tiles >> (8 + tt)) & 1) {
            if constexpr (BF16) {
              // accumulator register i is feature rho(i, h): four runs of 4 consecutive table entries
              const HnDFeat* dft = dfeat_lds + w[3] + 32 * tt + 4 * h;
              const char* srcv_r = reinterpret_cast<const char*>(srcv) + 4 * r;
#pragma unroll
              for (int q4 = 0; q4 < 4; ++q4) {
                float g[4];
                hn_feature_grads4(dft + 8 * q4, srcv_r, g);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * q4 + e] *= g[e];
              }
            } else {
#pragma unroll
              for (int i = 0; i < 16; ++i) acc[i] *= hn_feature_grad<BF16>(ft[hn_rho(i, h)], srcv, r);
            }
          }
          Frag gfr[M::STEPS32];
          hn_acc_to_frags(acc, gfr);
          hn_gemm_blocks<BF16, 1>(dacc, gfr, ws);
          HN_STAMP(5);
        }
      }
    }
    // source gradients of this block -> global
    if (a.n_dsrc > 0 && a.dsrc != nullptr && p0 < a.n_points) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int slot = hn_rho(i, h);
        if (slot < a.n_dsrc) a.dsrc[(size_t)p0 * a.n_dsrc + slot] = S8 ? dacc[i] * dz_unscale : dacc[i];
      }
    }
    // GLOEmbed backward (modules.py:155-167 under autograd): the block's 32 points belong to one ray, so the
    // gradient of the gathered row is the sum over the lanes of each half, added once per block and component
    if (a.embed_reg_mask != 0 && wave_valid) {
      const long long erow = a.embed_idx[(blk * 32) / a.samples_per_ray];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (a.embed_reg_mask & (1 << i)) {
          float v = valid ? (S8 ? dacc[i] * dz_unscale : dacc[i]) : 0.0f;
#pragma unroll
          for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m, 64);
          const int col = a.embed_col[hn_rho(i, h)];
          if (r == 0 && col >= 0) {
            // (the opt-in 8-bit-stash build keeps the atomics: the host never hands it a partial buffer, and the extra
            // pointer pushed that build's allocation into scratch)
            if (!S8 && a.embed_partial != nullptr) a.embed_partial[(size_t)blk * a.embed_dim + col] = v;
            else if (erow >= 0 && erow < a.embed_rows) atomicAdd(a.embed_grad + (size_t)erow * a.embed_dim + col, v);
          }
        }
      }
    }
  }
  hn_timeline_end(a.timeline);
