// The AgentAttention kernels that touch q, k, v, o, dO, dq, dk or dv, written once for both element types: agent.hip
// includes this file twice, with AGENT_E = float and AGENT_KERNEL(s2) = agent_s2_kernel<ints> (the names the f32
// kernels always had: what profiles and tests/agent_ref.py know), then with AGENT_E = __bf16 and AGENT_KERNEL(s2) =
// agent_s2_bf16_kernel<ints>.  Textual inclusion instead of a __device__ body template behind two __global__
// wrappers: a wrapper's loads reach the kernel only by inlining, after the pass that marks a kernel's unclobbered
// loads has run, and without those marks the compiler fuses other products of the streaming stage-2 backward into
// FMAs -- the f32 dq moved in its last bit against the build before.  Here the f32 kernels compile as they always did.
// Only the global accesses depend on E (bld4 / bst4 / gld4 / gst4 / row_off and the row helpers built on them): E =
// __bf16 widens exactly on the load and rounds to nearest even once, on the store; the arithmetic in between is f32 in
// one order for both.  No include guard: meant to be included more than once, inside namespace amk_agent.

// ---------------------------------------------------------------------------------------
// forward 0: agent tokens = mean of q over the adaptive bin (AdaptiveAvgPool2d over (t, h), h == p).
// One workgroup per (b, h, agent); RPP rows per pass.
template <int D>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(pool)(Params p) {
  using E = AGENT_E;
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) float red[4 * D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c4 = (tid & (C::LPR - 1)) * 4;
  const int i = blockIdx.x % p.P;
  const int bh = blockIdx.x / p.P;
  const int h = bh % p.H, b = bh / p.H;
  const E* qb = static_cast<const E*>(p.q) + (int64_t)b * p.qs.sb + (int64_t)h * p.qs.sh;
  const int lo = bin_lo(i, p.T, p.P), hi = bin_hi(i, p.T, p.P);
  float4 s = splat4(0.f);
  for (int t = lo + (tid >> C::LPR_LOG); t < hi; t += C::RPP) {
    const float4 x = gld4<E>(qb + (int64_t)t * p.qs.st + c4);
    s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
  }
  s = fold_subs<D>(s);
  if (lane < C::LPR) st4(&red[wave * D + c4], s);
  __syncthreads();
  if (wave == 0)
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D)
      p.agents[((int64_t)bh * p.P + i) * D + c] =
          (red[c] + red[D + c] + red[2 * D + c] + red[3 * D + c]) / (float)(hi - lo);
}

// forward 1: per-chunk partial of V_agent = softmax((A*scale) K^T) V: chunk max, chunk row sum and
// the un-normalised sum over the chunk's keys.
template <int D, int PM>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(s1_partial)(Params p) {
  using E = AGENT_E;
  using C = Cfg<D>;
  constexpr int CH = C::CH, TS = C::TS, PSTR = C::PSTR;
  __shared__ __attribute__((aligned(16))) float As[PM * D];
  __shared__ __attribute__((aligned(16))) float tile[CH * TS];   // k rows, then the cross-wave reduction
  __shared__ float S[PM * CH];
  __shared__ float mloc[PM], lloc[PM];
  float* red = tile;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Where w = where<CH>(p.H, p.NC);
  const int P = p.P, T = p.T, t0 = w.t0;
  const E* kb = static_cast<const E*>(p.k) + (int64_t)w.b * p.ks.sb + (int64_t)w.h * p.ks.sh;
  const E* vb = static_cast<const E*>(p.v) + (int64_t)w.b * p.vs.sb + (int64_t)w.h * p.vs.sh;

  for (int i = wave; i < P; i += 4)
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) As[i * D + c] = p.agents[(w.bh * P + i) * D + c] * p.scale;
  stage_rows<D, E>(tile, kb, p.ks.st, t0, T, tid);
  // the value rows of phase B (D / 4 lanes per row, RPP rows per pass) are requested NOW and arrive under phase A: the
  // barriers in between order LDS only
  const int sub = (tid >> C::LPR_LOG), c4 = (tid & (C::LPR - 1)) * 4;
  float4 vrow[C::NPIECE];
  {
    const __amdgpu_buffer_rsrc_t vrs = slab(vb);
#pragma unroll
    for (int j = 0; j < C::NPIECE; ++j) vrow[j] = bld4<E>(vrs, row_off<E>(t0 + C::RPP * j + sub, T, p.vs.st, c4));
  }
  lds_barrier();
  {  // phase A: TPT threads per key
    const int tok = tid >> C::TPT_LOG, half = tid & (C::TPT - 1);
    float kr[C::TCH];
    load_half<D>(tile, tok, half, kr);
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      if (i < P) {
        const float s = dot_half<D>(kr, &As[i * D], half);
        if (half == 0) S[i * CH + tok] = (t0 + tok < T) ? s : -INFINITY;
      }
    }
  }
  lds_barrier();
  for (int i = wave; i < P; i += 4) {  // chunk max per agent: one wave per agent
    float m = S[i * CH + lane];
#pragma unroll
    for (int r = 64; r < CH; r += 64) m = fmaxf(m, S[i * CH + r + lane]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) mloc[i] = m;  // finite: every chunk holds at least one key
  }
  lds_barrier();
  for (int e = tid; e < P * CH; e += NT) S[e] = expf(S[e] - mloc[e / CH]);   // (rows past T: exp(-inf) = 0)
  lds_barrier();
  {  // phase B: D / 4 lanes per value row, RPP rows of the chunk per pass
    float4 acc[PM];
#pragma unroll
    for (int i = 0; i < PM; ++i) acc[i] = splat4(0.f);
#pragma unroll
    for (int j = 0; j < C::NPIECE; ++j) {
      const int r = C::RPP * j + sub;
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) fma4(acc[i], S[i * CH + r], vrow[j]);
    }
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      if (i < P) {
        const float4 a = fold_subs<D>(acc[i]);
        if (lane < C::LPR) st4(&red[(wave * MAXP + i) * D + c4], a);
      }
    }
    for (int i = wave; i < P; i += 4) {  // row sums of this chunk, one wave per agent
      float s = S[i * CH + lane];
#pragma unroll
      for (int r = 64; r < CH; r += 64) s = s + S[i * CH + r + lane];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) lloc[i] = s;
    }
  }
  __syncthreads();
  for (int i = wave; i < P; i += 4) {
    float* rec = p.part + ((w.bh * p.NC + w.ch) * P + i) * PSTR;
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) rec[c] = fold4<D>(red, i, c);
    if (lane == 0) { rec[D] = mloc[i]; rec[D + 1] = lloc[i]; }
  }
}

// forward 3: O = softmax((q*scale) A^T) V_agent + dwc(v) for one chunk of tokens.
template <int D, int PM>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(s2)(Params p) {
  using E = AGENT_E;
  using C = Cfg<D>;
  constexpr int CH = C::CH, TS = C::TS;
  __shared__ __attribute__((aligned(16))) float As[PM * D];
  __shared__ __attribute__((aligned(16))) float tile[CH * TS];   // q rows
  __shared__ float S[PM * CH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Where w = where<CH>(p.H, p.NC);
  const int P = p.P, T = p.T, t0 = w.t0;
  const E* qb = static_cast<const E*>(p.q) + (int64_t)w.b * p.qs.sb + (int64_t)w.h * p.qs.sh;

  for (int i = wave; i < P; i += 4)
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) As[i * D + c] = p.agents[(w.bh * P + i) * D + c] * p.scale;
  stage_rows<D, E>(tile, qb, p.qs.st, t0, T, tid);
  // phase B mapping: D / 4 lanes per output row, and a lane group takes CH / RPP CONSECUTIVE rows, so that the 3x3
  // window of the depthwise convolution slides: three new value rows (heads h-1, h, h+1) per output row instead of
  // nine.  The first rows of the window are requested now and arrive under phase A (LDS-only barriers in between).
  constexpr int RPG = C::NPIECE;   // rows per group
  const int grp = (tid >> C::LPR_LOG), c4 = (tid & (C::LPR - 1)) * 4;
  const __amdgpu_buffer_rsrc_t vrs = slab(static_cast<const E*>(p.v) + (int64_t)w.b * p.vs.sb);
  auto ldv = [&](int a, int t) {   // value row of head h + a - 1 at token t, channels c4..c4+3; zero padding
    const int h2 = w.h + a - 1;
    return bld4<E>(vrs, (h2 >= 0 && h2 < p.H && t >= 0 && t < T) ? (unsigned)(((int64_t)h2 * p.vs.sh + (int64_t)t * p.vs.st + c4) * (int)sizeof(E)) : PAST);
  };
  const int tfirst = t0 + RPG * grp;
  float4 win[3][4];   // [head offset][token slot]: tokens t-1, t, t+1 and the prefetched t+2
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    win[a][0] = ldv(a, tfirst - 1); win[a][1] = ldv(a, tfirst); win[a][2] = ldv(a, tfirst + 1); win[a][3] = ldv(a, tfirst + 2);
  }
  lds_barrier();
  {  // phase A: TPT threads per token: p scores, softmax over the agents
    const int tok = tid >> C::TPT_LOG, half = tid & (C::TPT - 1);
    float qr[C::TCH];
    load_half<D>(tile, tok, half, qr);
    float sc[PM];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < PM; ++i)
      if (i < P) { sc[i] = dot_half<D>(qr, &As[i * D], half); m = fmaxf(m, sc[i]); }
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < PM; ++i)
      if (i < P) { sc[i] = expf(sc[i] - m); l += sc[i]; }
    if (half == 0) {
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) S[i * CH + tok] = sc[i] / l;
    }
  }
  lds_barrier();
  {  // phase B
    float4 wq[9], var[PM];
    load_taps(p.convw, c4, wq);
    const float4 cb = ld4(p.convb + c4);
#pragma unroll
    for (int i = 0; i < PM; ++i) var[i] = (i < P) ? ld4(p.vagent + (w.bh * P + i) * D + c4) : splat4(0.f);
    const __amdgpu_buffer_rsrc_t ors = slab(static_cast<E*>(p.o) + (int64_t)w.b * p.os.sb + (int64_t)w.h * p.os.sh);
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      const int r = RPG * grp + j, t = t0 + r;
      float4 o = cb;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) mad4(o, wq[a * 3 + b], win[a][b]);
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) fma4(o, S[i * CH + r], var[i]);
      bst4<E>(ors, row_off<E>(t, T, p.os.st, c4), o);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        win[a][0] = win[a][1]; win[a][1] = win[a][2]; win[a][2] = win[a][3];
        win[a][3] = ldv(a, (j + 3 <= RPG) ? t + 3 : -1);   // (row t+3 is the last one the group's window needs)
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// backward 0: stage-2 backward of one chunk: dq (broadcast part), partials of dV_agent, of dA
// (broadcast part) and of the conv weight / bias gradients.
template <int D, int PM>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(s2_bwd)(BwdParams p) {
  using E = AGENT_E;
  using C = Cfg<D>;
  constexpr int CH = C::CH, TS = C::TS, HALF = C::TCH;
  __shared__ __attribute__((aligned(16))) float As[PM * D];
  __shared__ __attribute__((aligned(16))) float Vas[PM * D];
  __shared__ __attribute__((aligned(16))) float tile[CH * TS];   // q rows, dO rows, dq rows out, reductions
  __shared__ float S[PM * CH];    // P2 of the chunk
  __shared__ float DS[PM * CH];   // dS2 of the chunk
  float* red = tile;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Where w = where<CH>(p.H, p.NC);
  const int P = p.P, T = p.T, t0 = w.t0, h = w.h;
  const E* qb = static_cast<const E*>(p.q) + (int64_t)w.b * p.qs.sb + (int64_t)h * p.qs.sh;
  const E* gb = static_cast<const E*>(p.d_o) + (int64_t)w.b * p.dos.sb + (int64_t)h * p.dos.sh;
  float* dqb = dq_part<D, E>(p, w);
  const E* vbatch = static_cast<const E*>(p.v) + (int64_t)w.b * p.vs.sb;

  AG_STAMP(0);
  for (int i = wave; i < P; i += 4) {
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) {
      As[i * D + c] = p.agents[(w.bh * P + i) * D + c];
      Vas[i * D + c] = p.vagent[(w.bh * P + i) * D + c];
    }
  }
  stage_rows<D, E>(tile, qb, p.qs.st, t0, T, tid);
  float4 gpc[C::NPIECE];
  fetch_rows<D, E>(gpc, gb, p.dos.st, t0, T, tid);   // the dO tile: in flight while the q tile is worked on
  // phase B (below): D / 4 lanes per row, a lane group takes CH / RPP CONSECUTIVE rows: the 3x3 window of value rows behind
  // the convolution's weight gradient slides (three new rows per token instead of nine), rows two tokens ahead in
  // flight; its first rows are requested here, a whole phase early
  constexpr int RPG = C::NPIECE;
  const int grp = (tid >> C::LPR_LOG), c4 = (tid & (C::LPR - 1)) * 4;
  const __amdgpu_buffer_rsrc_t vrs = slab(vbatch), grs = slab(gb), qrs = slab(qb);
  auto ldv = [&](int a, int t) {
    const int h2 = h + a - 1;
    return bld4<E>(vrs, (h2 >= 0 && h2 < p.H && t >= 0 && t < T) ? (unsigned)(((int64_t)h2 * p.vs.sh + (int64_t)t * p.vs.st + c4) * (int)sizeof(E)) : PAST);
  };
  const int tfirst = t0 + RPG * grp;
  float4 win[3][4], gq[2][3];   // value window [head offset][t-1, t, t+1, t+2]; dO / q rows [t, t+1, t+2]
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    win[a][0] = ldv(a, tfirst - 1); win[a][1] = ldv(a, tfirst); win[a][2] = ldv(a, tfirst + 1); win[a][3] = ldv(a, tfirst + 2);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { gq[0][k] = bld4<E>(grs, row_off<E>(tfirst + k, T, p.dos.st, c4)); gq[1][k] = bld4<E>(qrs, row_off<E>(tfirst + k, T, p.qs.st, c4)); }
  lds_barrier();
  AG_STAMP(1);
  {  // phase A: TPT threads per token
    const int tok = tid >> C::TPT_LOG, half = tid & (C::TPT - 1);
    const bool ok = t0 + tok < T;
    float sc[PM], dp[PM];
    {
      float qr[HALF];
      load_half<D>(tile, tok, half, qr);
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) sc[i] = dot_half<D>(qr, &As[i * D], half) * p.scale;
    }
    lds_barrier();
    put_rows<D>(tile, gpc, tid);
    lds_barrier();
    AG_STAMP(2);
    {
      float gr[HALF];
      load_half<D>(tile, tok, half, gr);
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) dp[i] = dot_half<D>(gr, &Vas[i * D], half);
    }
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < PM; ++i)
      if (i < P) m = fmaxf(m, sc[i]);
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < PM; ++i)
      if (i < P) { sc[i] = expf(sc[i] - m); l += sc[i]; }
    float dl = 0.f;
#pragma unroll
    for (int i = 0; i < PM; ++i)
      if (i < P) { sc[i] /= l; dl += sc[i] * dp[i]; }
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      if (i < P) {
        const float ds = sc[i] * (dp[i] - dl);
        if (half == 0) {
          S[i * CH + tok] = ok ? sc[i] : 0.f;
          DS[i * CH + tok] = ok ? ds : 0.f;
        }
        dp[i] = ds * p.scale;
      }
    }
    // dq_t = scale * sum_i dS2[t,i] A_i: this thread's 32 channels into its own half row of the tile
    float* dst = tile + tok * TS + HALF * half;
#pragma unroll
    for (int j = 0; j < HALF / 4; ++j) {
      float4 o = splat4(0.f);
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) fma4(o, dp[i], ld4(&As[i * D + HALF * half + 4 * j]));
      st4(dst + 4 * j, o);
    }
  }
  __syncthreads();
  AG_STAMP(3);
  unstage_rows<D, float>(tile, dqb, dq_part_st<D, E>(p), t0, T, tid);
  float4 accva[PM], acca[PM], dw9[9], dbs = splat4(0.f);
#pragma unroll
  for (int i = 0; i < PM; ++i) { accva[i] = splat4(0.f); acca[i] = splat4(0.f); }
#pragma unroll
  for (int j = 0; j < 9; ++j) dw9[j] = splat4(0.f);
  {
#pragma unroll 1
    for (int j = 0; j < RPG; ++j) {
      const int r = RPG * grp + j, t = t0 + r;
      const float4 g = gq[0][0], qv = gq[1][0];   // (rows past T: zeros, and S / DS are zero there)
#pragma unroll
      for (int i = 0; i < PM; ++i) {
        if (i < P) {
          fma4(accva[i], S[i * CH + r], g);
          fma4(acca[i], DS[i * CH + r], qv);
        }
      }
      dbs.x += g.x; dbs.y += g.y; dbs.z += g.z; dbs.w += g.w;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int bb = 0; bb < 3; ++bb) mad4(dw9[a * 3 + bb], g, win[a][bb]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        win[a][0] = win[a][1]; win[a][1] = win[a][2]; win[a][2] = win[a][3];
        win[a][3] = ldv(a, (j + 3 <= RPG) ? t + 3 : -1);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        gq[k][0] = gq[k][1]; gq[k][1] = gq[k][2];
        gq[k][2] = bld4<E>(k == 0 ? grs : qrs, (j + 3 < RPG) ? row_off<E>(t + 3, T, k == 0 ? p.dos.st : p.qs.st, c4) : PAST);
      }
    }
  }
  const int64_t cell = w.bh * p.NC + w.ch;
  AG_STAMP(4);
  __syncthreads();  // the dq rows have left the tile
#pragma unroll
  for (int i = 0; i < PM; ++i) {
    if (i < P) {
      const float4 a = fold_subs<D>(accva[i]);
      if (lane < C::LPR) st4(&red[(wave * MAXP + i) * D + c4], a);
    }
  }
  __syncthreads();
  for (int i = wave; i < P; i += 4)
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) p.pva[(cell * P + i) * D + c] = fold4<D>(red, i, c);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PM; ++i) {
    if (i < P) {
      const float4 a = fold_subs<D>(acca[i]);
      if (lane < C::LPR) st4(&red[(wave * MAXP + i) * D + c4], a);
    }
  }
  __syncthreads();
  for (int i = wave; i < P; i += 4)
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) p.pa2[(cell * P + i) * D + c] = p.scale * fold4<D>(red, i, c);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const float4 a = fold_subs<D>(dw9[j]);
    if (lane < C::LPR) st4(&red[(wave * MAXP + j) * D + c4], a);
  }
  {
    const float4 a = fold_subs<D>(dbs);
    if (lane < C::LPR) st4(&red[(wave * MAXP + 9) * D + c4], a);
  }
  __syncthreads();
  if (wave == 0) {
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) {
      for (int j = 0; j < 9; ++j) p.dconvw_part[(cell * 9 + j) * D + c] = fold4<D>(red, j, c);
      p.dconvb_part[cell * D + c] = fold4<D>(red, 9, c);
    }
  }
  AG_STAMP(5);
}

// backward 2: stage-1 backward of one chunk: dk, dv (aggregation + transposed conv of dO), partial
// of dA (aggregation part).
template <int D, int PM>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(s1_bwd)(BwdParams p) {
  using E = AGENT_E;
  using C = Cfg<D>;
  constexpr int CH = C::CH, TS = C::TS, HALF = C::TCH;
  __shared__ __attribute__((aligned(16))) float As[PM * D];
  __shared__ __attribute__((aligned(16))) float dVas[PM * D];
  __shared__ __attribute__((aligned(16))) float tile[CH * TS];   // k rows, v rows, dk rows out, reduction
  __shared__ float S[PM * CH];    // P1 of the chunk
  __shared__ float DS[PM * CH];   // dS1 of the chunk
  __shared__ float m1[PM], l1[PM], delta1[PM];
  float* red = tile;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Where w = where<CH>(p.H, p.NC);
  const int P = p.P, T = p.T, t0 = w.t0, h = w.h;
  const E* kb = static_cast<const E*>(p.k) + (int64_t)w.b * p.ks.sb + (int64_t)h * p.ks.sh;
  const E* vb = static_cast<const E*>(p.v) + (int64_t)w.b * p.vs.sb + (int64_t)h * p.vs.sh;
  E* dkb = static_cast<E*>(p.dk) + (int64_t)w.b * p.dks.sb + (int64_t)h * p.dks.sh;
  E* dvb = static_cast<E*>(p.dv) + (int64_t)w.b * p.dvs.sb + (int64_t)h * p.dvs.sh;
  const E* gbatch = static_cast<const E*>(p.d_o) + (int64_t)w.b * p.dos.sb;

  for (int i = wave; i < P; i += 4) {
    const int64_t row = w.bh * P + i;
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) {
      As[i * D + c] = p.agents[row * D + c];
      dVas[i * D + c] = p.dva[row * D + c];
    }
    if (lane == 0) { m1[i] = p.stats1[row * 2]; l1[i] = p.stats1[row * 2 + 1]; delta1[i] = p.delta1[row]; }
  }
  stage_rows<D, E>(tile, kb, p.ks.st, t0, T, tid);
  float4 vpc[C::NPIECE];
  fetch_rows<D, E>(vpc, vb, p.vs.st, t0, T, tid);   // the v tile: in flight while the k tile is worked on
  lds_barrier();
  {  // phase A: TPT threads per key
    const int tok = tid >> C::TPT_LOG, half = tid & (C::TPT - 1);
    const bool ok = t0 + tok < T;
    float pr[PM], ds[PM];
    {
      float kr[HALF];
      load_half<D>(tile, tok, half, kr);
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) pr[i] = expf(dot_half<D>(kr, &As[i * D], half) * p.scale - m1[i]) / l1[i];
    }
    lds_barrier();
    put_rows<D>(tile, vpc, tid);
    lds_barrier();
    {
      float vr[HALF];
      load_half<D>(tile, tok, half, vr);
#pragma unroll
      for (int i = 0; i < PM; ++i) {
        if (i < P) {
          const float dp = dot_half<D>(vr, &dVas[i * D], half);
          const float d = pr[i] * (dp - delta1[i]);
          if (half == 0) {
            S[i * CH + tok] = ok ? pr[i] : 0.f;
            DS[i * CH + tok] = ok ? d : 0.f;
          }
          ds[i] = d * p.scale;
        }
      }
    }
    // dk_t = scale * sum_i dS1[i,t] A_i
    float* dst = tile + tok * TS + HALF * half;
#pragma unroll
    for (int j = 0; j < HALF / 4; ++j) {
      float4 o = splat4(0.f);
#pragma unroll
      for (int i = 0; i < PM; ++i)
        if (i < P) fma4(o, ds[i], ld4(&As[i * D + HALF * half + 4 * j]));
      st4(dst + 4 * j, o);
    }
  }
  __syncthreads();
  unstage_rows<D, E>(tile, dkb, p.dks.st, t0, T, tid);
  // phase B: D / 4 lanes per row, CH / RPP consecutive rows per lane group: the 3x3 window of dO rows behind the
  // transposed depthwise convolution slides (three new rows per token instead of nine)
  constexpr int RPG = C::NPIECE;
  const int grp = (tid >> C::LPR_LOG), c4 = (tid & (C::LPR - 1)) * 4;
  float4 acca[PM];
  {
    float4 wq[9], dva[PM];
    load_taps(p.convw, c4, wq);
#pragma unroll
    for (int i = 0; i < PM; ++i) { acca[i] = splat4(0.f); dva[i] = (i < P) ? ld4(&dVas[i * D + c4]) : splat4(0.f); }
    // dv[h, t] += sum_{a, b} w[a][b] dO[h - (a - 1), t - (b - 1)]: window slot s holds dO[., t - 1 + s] of head h + 1 - a
    const __amdgpu_buffer_rsrc_t grs = slab(gbatch), krs = slab(kb), dvrs = slab(dvb);
    auto ldg = [&](int a, int t) {
      const int h2 = h - (a - 1);
      return bld4<E>(grs, (h2 >= 0 && h2 < p.H && t >= 0 && t < T) ? (unsigned)(((int64_t)h2 * p.dos.sh + (int64_t)t * p.dos.st + c4) * (int)sizeof(E)) : PAST);
    };
    const int tfirst = t0 + RPG * grp;
    float4 win[3][4], krow[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      win[a][0] = ldg(a, tfirst - 1); win[a][1] = ldg(a, tfirst); win[a][2] = ldg(a, tfirst + 1); win[a][3] = ldg(a, tfirst + 2);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) krow[k] = bld4<E>(krs, row_off<E>(tfirst + k, T, p.ks.st, c4));
#pragma unroll 1
    for (int j = 0; j < RPG; ++j) {
      const int r = RPG * grp + j, t = t0 + r;
      const float4 kv = krow[0];
      float4 dvv = splat4(0.f);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int bb = 0; bb < 3; ++bb) mad4(dvv, wq[a * 3 + bb], win[a][2 - bb]);   // token t - (bb - 1) = slot 2 - bb
#pragma unroll
      for (int i = 0; i < PM; ++i) {
        if (i < P) {
          fma4(acca[i], DS[i * CH + r], kv);
          fma4(dvv, S[i * CH + r], dva[i]);
        }
      }
      bst4<E>(dvrs, row_off<E>(t, T, p.dvs.st, c4), dvv);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        win[a][0] = win[a][1]; win[a][1] = win[a][2]; win[a][2] = win[a][3];
        win[a][3] = ldg(a, (j + 3 <= RPG) ? t + 3 : -1);
      }
      krow[0] = krow[1]; krow[1] = krow[2];
      krow[2] = bld4<E>(krs, (j + 3 < RPG) ? row_off<E>(t + 3, T, p.ks.st, c4) : PAST);
    }
  }
  __syncthreads();  // the dk rows have left the tile
#pragma unroll
  for (int i = 0; i < PM; ++i) {
    if (i < P) {
      const float4 a = fold_subs<D>(acca[i]);
      if (lane < C::LPR) st4(&red[(wave * MAXP + i) * D + c4], a);
    }
  }
  __syncthreads();
  const int64_t cell = w.bh * p.NC + w.ch;
  for (int i = wave; i < P; i += 4)
    for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) p.pa1[(cell * P + i) * D + c] = p.scale * fold4<D>(red, i, c);
}

template <int PM>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(s2_bwd_stream)(BwdParams p) {
  using E = AGENT_E;
  constexpr int D = 64, CH = Cfg<D>::CH;   // streaming forms: head dim 64 only
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * PM * D];   // [wave][dV_agent | dA][agent][channel]
  constexpr int RPG = CH / (NT / 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, c4 = (tid & 15) * 4;
  const Where w = where<CH>(p.H, p.NC);
  const int P = p.P, T = p.T, h = w.h;
  const __amdgpu_buffer_rsrc_t qrs = slab(static_cast<const E*>(p.q) + (int64_t)w.b * p.qs.sb + (int64_t)h * p.qs.sh);
  const __amdgpu_buffer_rsrc_t grs = slab(static_cast<const E*>(p.d_o) + (int64_t)w.b * p.dos.sb + (int64_t)h * p.dos.sh);
  const __amdgpu_buffer_rsrc_t dqrs = slab(dq_part<D, E>(p, w));
  const int tfirst = w.t0 + RPG * grp;
  float4 qg[2][4];   // q / dO rows [t, t+1, t+2, t+3]: three rows of requests in flight ahead of the one being worked on
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    qg[0][k] = bld4<E>(qrs, row_off<E>(tfirst + k, T, p.qs.st, c4));
    qg[1][k] = bld4<E>(grs, row_off<E>(tfirst + k, T, p.dos.st, c4));
  }
  float4 A[PM], Va[PM], accva[PM], acca[PM];
#pragma unroll
  for (int i = 0; i < PM; ++i) {
    A[i] = i < P ? ld4(p.agents + (w.bh * P + i) * D + c4) : splat4(0.f);
    Va[i] = i < P ? ld4(p.vagent + (w.bh * P + i) * D + c4) : splat4(0.f);
    accva[i] = splat4(0.f); acca[i] = splat4(0.f);
  }
#pragma unroll 1
  for (int j = 0; j < RPG; ++j) {
    const float4 qv = qg[0][0], g = qg[1][0];
    const bool ok = tfirst + j < T;
    float sc[PM], dp[PM];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      sc[i] = fold16(dot4(qv, A[i])) * p.scale;
      dp[i] = fold16(dot4(g, Va[i]));
      if (i < P) m = fmaxf(m, sc[i]);
    }
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < PM; ++i) { sc[i] = i < P ? expf(sc[i] - m) : 0.f; l += sc[i]; }
    const float il = ok ? 1.f / l : 0.f;   // (rows past the sequence: P2 = 0, dS2 = 0)
    float dl = 0.f;
#pragma unroll
    for (int i = 0; i < PM; ++i) { sc[i] *= il; dl += sc[i] * dp[i]; }
    float4 dq = splat4(0.f);
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      const float ds = sc[i] * (dp[i] - dl);
      fma4(dq, ds * p.scale, A[i]);
      fma4(accva[i], sc[i], g);
      fma4(acca[i], ds, qv);
    }
    bst4<float>(dqrs, row_off<float>(tfirst + j, T, dq_part_st<D, E>(p), c4), dq);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      qg[k][0] = qg[k][1]; qg[k][1] = qg[k][2]; qg[k][2] = qg[k][3];
      qg[k][3] = bld4<E>(k == 0 ? qrs : grs, (j + 4 < RPG) ? row_off<E>(tfirst + j + 4, T, k == 0 ? p.qs.st : p.dos.st, c4) : PAST);
    }
  }
  // fold the 16 groups: 4 per wave by DPP, the 4 waves through LDS
#pragma unroll
  for (int i = 0; i < PM; ++i) {
    if (i < P) {
      const float4 a = fold_subs<D>(accva[i]), b = fold_subs<D>(acca[i]);
      if (lane < 16) { st4(&red[((wave * 2 + 0) * PM + i) * D + c4], a); st4(&red[((wave * 2 + 1) * PM + i) * D + c4], b); }
    }
  }
  __syncthreads();
  const int64_t cell = w.bh * p.NC + w.ch;
  for (int i = wave; i < P; i += 4) {
    float sva = 0.f, sa = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) { sva += red[((ww * 2 + 0) * PM + i) * D + lane]; sa += red[((ww * 2 + 1) * PM + i) * D + lane]; }
    p.pva[(cell * P + i) * D + lane] = sva;
    p.pa2[(cell * P + i) * D + lane] = p.scale * sa;
  }
}

template <int PM>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(s1_bwd_stream)(BwdParams p) {
  using E = AGENT_E;
  constexpr int D = 64, CH = Cfg<D>::CH;
  __shared__ __attribute__((aligned(16))) float red[4 * (PM + 10) * D];   // [wave][dA (PM) | dconv_w (9) | dconv_b][channel]
  __shared__ __attribute__((aligned(16))) float wqs[9 * D];                // the convolution's taps [tap][channel]
  __shared__ __attribute__((aligned(16))) float As[PM * D], dVas[PM * D];  // agents and dV_agent: 48 registers too many next
                                                                           // to the 36 of the convolution's gradient
  __shared__ float m1[PM], il1[PM], delta1[PM];
  constexpr int RPG = CH / (NT / 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, c4 = (tid & 15) * 4;
  const Where w = where<CH>(p.H, p.NC);
  const int P = p.P, T = p.T, h = w.h;
  const __amdgpu_buffer_rsrc_t krs = slab(static_cast<const E*>(p.k) + (int64_t)w.b * p.ks.sb + (int64_t)h * p.ks.sh);
  const __amdgpu_buffer_rsrc_t vrs = slab(static_cast<const E*>(p.v) + (int64_t)w.b * p.vs.sb + (int64_t)h * p.vs.sh);
  const __amdgpu_buffer_rsrc_t grs = slab(static_cast<const E*>(p.d_o) + (int64_t)w.b * p.dos.sb);
  const __amdgpu_buffer_rsrc_t dkrs = slab(static_cast<E*>(p.dk) + (int64_t)w.b * p.dks.sb + (int64_t)h * p.dks.sh);
  const __amdgpu_buffer_rsrc_t dvrs = slab(static_cast<E*>(p.dv) + (int64_t)w.b * p.dvs.sb + (int64_t)h * p.dvs.sh);
  const int tfirst = w.t0 + RPG * grp;
  // dO rows of head h - (a - 1) at token t (zero padding): the window of the transposed depthwise convolution
  auto ldg = [&](int a, int t) {
    const int h2 = h - (a - 1);
    return bld4<E>(grs, (h2 >= 0 && h2 < p.H && t >= 0 && t < T) ? (unsigned)(((int64_t)h2 * p.dos.sh + (int64_t)t * p.dos.st + c4) * (int)sizeof(E)) : PAST);
  };
  float4 win[3][4], kv[2][3];   // dO window [head offset][t-1, t, t+1, t+2]; k / v rows [t, t+1, t+2]
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    win[a][0] = ldg(a, tfirst - 1); win[a][1] = ldg(a, tfirst); win[a][2] = ldg(a, tfirst + 1); win[a][3] = ldg(a, tfirst + 2);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { kv[0][k] = bld4<E>(krs, row_off<E>(tfirst + k, T, p.ks.st, c4)); kv[1][k] = bld4<E>(vrs, row_off<E>(tfirst + k, T, p.vs.st, c4)); }
  if (tid < 9 * 16) {   // taps: wqs[j][c] = convw[c][j]
    const int j = tid / 16, cc = (tid & 15) * 4;
    st4(&wqs[j * D + cc], make_float4(p.convw[(cc + 0) * 9 + j], p.convw[(cc + 1) * 9 + j], p.convw[(cc + 2) * 9 + j], p.convw[(cc + 3) * 9 + j]));
  }
  if (tid < P) {
    const int64_t row = w.bh * P + tid;
    m1[tid] = p.stats1[row * 2]; il1[tid] = 1.f / p.stats1[row * 2 + 1]; delta1[tid] = p.delta1[row];
  }
  for (int i = wave; i < P; i += 4) {
    As[i * D + lane] = p.agents[(w.bh * P + i) * D + lane];
    dVas[i * D + lane] = p.dva[(w.bh * P + i) * D + lane];
  }
  float4 acca[PM], dw9[9], dbs = splat4(0.f);
#pragma unroll
  for (int i = 0; i < PM; ++i) acca[i] = splat4(0.f);
#pragma unroll
  for (int j = 0; j < 9; ++j) dw9[j] = splat4(0.f);
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < RPG; ++j) {
    const int t = tfirst + j;
    const float4 kr = kv[0][0], vr = kv[1][0];
    const bool ok = t < T;
    float4 dk = splat4(0.f), dvv = splat4(0.f);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bb = 0; bb < 3; ++bb) {
        mad4(dvv, ld4(&wqs[(a * 3 + bb) * D + c4]), win[a][2 - bb]);   // dv[h, t] += w[a][b] dO[h - (a-1), t - (b-1)]
        mad4(dw9[a * 3 + bb], vr, win[a][2 - bb]);                      // (v is zero past the sequence)
      }
    dbs.x += win[1][1].x; dbs.y += win[1][1].y; dbs.z += win[1][1].z; dbs.w += win[1][1].w;   // dO[h, t]
#pragma unroll
    for (int i = 0; i < PM; ++i) {
      if (i < P) {
        const float4 Ai = ld4(&As[i * D + c4]), dVi = ld4(&dVas[i * D + c4]);
        const float s = fold16(dot4(kr, Ai)), dp = fold16(dot4(vr, dVi));
        const float pr = ok ? expf(s * p.scale - m1[i]) * il1[i] : 0.f;
        const float ds = pr * (dp - delta1[i]);
        fma4(dk, ds * p.scale, Ai);
        fma4(dvv, pr, dVi);
        fma4(acca[i], ds, kr);
      }
    }
    bst4<E>(dkrs, row_off<E>(t, T, p.dks.st, c4), dk);
    bst4<E>(dvrs, row_off<E>(t, T, p.dvs.st, c4), dvv);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      win[a][0] = win[a][1]; win[a][1] = win[a][2]; win[a][2] = win[a][3];
      win[a][3] = ldg(a, (j + 3 <= RPG) ? t + 3 : -1);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      kv[k][0] = kv[k][1]; kv[k][1] = kv[k][2];
      kv[k][2] = bld4<E>(k == 0 ? krs : vrs, (j + 3 < RPG) ? row_off<E>(t + 3, T, k == 0 ? p.ks.st : p.vs.st, c4) : PAST);
    }
  }
#pragma unroll
  for (int i = 0; i < PM; ++i) {
    if (i < P) {
      const float4 a = fold_subs<D>(acca[i]);
      if (lane < 16) st4(&red[(wave * (PM + 10) + i) * D + c4], a);
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const float4 a = fold_subs<D>(dw9[j]);
    if (lane < 16) st4(&red[(wave * (PM + 10) + PM + j) * D + c4], a);
  }
  {
    const float4 a = fold_subs<D>(dbs);
    if (lane < 16) st4(&red[(wave * (PM + 10) + PM + 9) * D + c4], a);
  }
  __syncthreads();
  const int64_t cell = w.bh * p.NC + w.ch;
  auto fold = [&](int slot) {
    float x = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) x += red[(ww * (PM + 10) + slot) * D + lane];
    return x;
  };
  for (int i = wave; i < P; i += 4) p.pa1[(cell * P + i) * D + lane] = p.scale * fold(i);
  for (int j = wave; j < 10; j += 4) {
    if (j < 9) p.dconvw_part[(cell * 9 + j) * D + lane] = fold(PM + j);
    else p.dconvb_part[cell * D + lane] = fold(PM + 9);
  }
}

// backward 3: dq[b,h,t,:] += sum over the bins i containing t of dA[b,h,i,:] / len(bin i) (E = __bf16: dq = the f32
// stage-2 part in dqf + that sum, rounded on the store), with
// dA = dA(stage 2) + the chunk partials of dA(stage 1) folded in chunk order.  One workgroup per
// (b, h, 64-token block): dA / len of the bins that meet the block is rebuilt in LDS first.
template <int D>
__global__ __launch_bounds__(NT) void AGENT_KERNEL(pool_bwd)(BwdParams p) {
  using E = AGENT_E;
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) float dA[MAXP * D];
  __shared__ int lo_s[MAXP], hi_s[MAXP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.T, P = p.P;
  const int nblk = (T + PB - 1) / PB;
  const int blk = blockIdx.x % nblk;
  const int64_t bh = blockIdx.x / nblk;
  const int h = (int)(bh % p.H), b = (int)(bh / p.H);
  const int t0 = blk * PB, t1 = min(T, t0 + PB);
  for (int i = wave; i < P; i += 4) {
    const int lo = bin_lo(i, T, P), hi = bin_hi(i, T, P);
    if (lane == 0) { lo_s[i] = lo; hi_s[i] = hi; }
    if (lo < t1 && hi > t0) {
      for (int k = 0; k < (D + 63) / 64; ++k) if (const int c = lane + 64 * k; D >= 64 || c < D) {
        float da = p.da2[(bh * P + i) * D + c];
        for (int ch = 0; ch < p.NC; ++ch) da += p.pa1[(((bh * p.NC + ch) * P) + i) * D + c];
        dA[i * D + c] = da / (float)(hi - lo);
      }
    }
  }
  __syncthreads();
  const int c4 = (tid & (C::LPR - 1)) * 4;
  E* dqb = static_cast<E*>(p.dq) + (int64_t)b * p.dqs.sb + (int64_t)h * p.dqs.sh;
#pragma unroll
  for (int r0 = 0; r0 < PB; r0 += C::RPP) {
    const int t = t0 + r0 + (tid >> C::LPR_LOG);
    if (t < T) {
      float4 add = splat4(0.f);
      for (int i = 0; i < P; ++i)
        if (t >= lo_s[i] && t < hi_s[i]) fma4(add, 1.f, ld4(&dA[i * D + c4]));
      E* dst = dqb + (int64_t)t * p.dqs.st + c4;
      const float4 cur = ld4(dq_part_row<D, E>(p, dst, bh * T + t, c4));
      gst4<E>(dst, make_float4(cur.x + add.x, cur.y + add.y, cur.z + add.z, cur.w + add.w));
    }
  }
}
