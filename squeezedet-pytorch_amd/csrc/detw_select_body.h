// Steps 1-4 of a wide select launch, as text: the radix select of the K-th key, the ordered sweep, the ranking and the decode of the
// <= K candidates.  Included -- not called -- by detect_wide_select_kernel (hard class-wise NMS on the bit matrix) and by
// detect_nms_select_kernel (the sequential scan of the other modes), inside the kernel body: a device function, however it was shaped,
// came out of the inliner with another instruction order and register assignment than the kernel had (same instructions, five fewer),
// and the wide kernels' device code is held byte-identical across this change (profiles/nms_modes_device_asm_diff.log).
// The including kernel provides: `a` (DetArgs), K, Kp = ceil64(K), the LDS arrays cand [Kp], boxL [Kp], clsL [Kp], hist [256],
// wave_tot [16], sv [4], the template parameter MANY (the many-class decode: a 16-lane group per candidate) and the macro
// DETW_PAD_ANY -- true: the words A .. ceil4(A)-1 of an image's key row may hold anything (keys written by ConvDet's epilogue) and are
// read as 0; false: the scoring launch wrote them as 0.  Every thread of the 1024-thread workgroup runs it.  It leaves in scope:
// tid, lane, wave, b, A, C, ncand, and for thread r < ncand (ok) the candidate of rank r: score, cls, idx, bx; boxL / clsL hold all
// of them in rank order (clsL = -1, boxL = 0 from ncand up to Kp).
// DETW_VIEWS (off for those two kernels; detect_views_select_kernel defines it as its view count, with DETW_VIEW_XF = the view table
// [B * V][6]): the pooled-views form of DESIGN.md section 3 "Pooled views" -- steps 1-3 run over the V key rows of the image as one
// row, step 4 maps every box into image coordinates; pred only, no dense inputs.
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)blockIdx.x;
#ifdef DETW_VIEWS
  // pooled views: the key rows of the image's V views, ceil4(A) words each, lie back to back and ARE one row of V * ceil4(A) words
  // (the scoring launch wrote every pad word as 0); a candidate's index below is s = v * ceil4(A) + anchor, ascending in (v, anchor)
  const int A = a.A, C = a.C, A4 = (A + 3) & ~3, nq = ((DETW_VIEWS) * A4) >> 2;
  const u32x4_w* __restrict__ ws4 = (const u32x4_w*)(a.keys + (long long)b * (DETW_VIEWS) * A4);
#else
  const int A = a.A, C = a.C, A4 = (A + 3) & ~3, nq = A4 >> 2;
  const u32x4_w* __restrict__ ws4 = (const u32x4_w*)(a.keys + (long long)b * A4);
#endif
  const bool dense = a.in_score != nullptr;

  if (tid == 0) { sv[0] = 0u; sv[1] = (unsigned)K; sv[2] = 0u; }
  if (tid < Kp) { clsL[tid] = -1; boxL[tid] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  __syncthreads();

  // 1. radix select of the K-th largest key among the M non-zero keys (pass 0 counts M)
  unsigned mask = 0u, M = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = sv[0];
    for (int q0 = 0; q0 < nq; q0 += DETW_THREADS) {
      const int q = q0 + tid;
      u32x4_w v = (u32x4_w){0u, 0u, 0u, 0u};
      if (q < nq) v = ws4[q];
      if (DETW_PAD_ANY && q == nq - 1) { if (A4 - A > 2) v.y = 0u; if (A4 - A > 1) v.z = 0u; if (A4 - A > 0) v.w = 0u; }
      const unsigned ks[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) detw_hist_add(hist, ks[e] != 0u && (ks[e] & mask) == prefix, (ks[e] >> shift) & 255u, lane);
    }
    __syncthreads();
    const unsigned need = sv[1];
    const unsigned h = (tid < 256) ? hist[255 - tid] : 0u;     // thread t owns bin 255 - t: the scan counts the keys in higher bins
    unsigned tot;
    const unsigned above = detw_excl_scan(h, tot, wave_tot, lane, wave);
    if (pass == 0) { M = tot; if (M <= (unsigned)K) break; }   // (uniform) every candidate is taken
    if (tid < 256 && above < need && above + h >= need) {      // exactly one thread
      sv[1] = need - above;
      sv[0] = prefix | ((unsigned)(255 - tid) << shift);
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  const bool sel = M > (unsigned)K;
  const unsigned tkey = sel ? sv[0] : 0u;                      // K-th largest key (>= 1), or 0: take every non-zero key
  const unsigned need = sel ? sv[1] : 0u;                      // keys == tkey to take, in ascending anchor order
  const unsigned n_gt = sel ? (unsigned)K - need : M;
  const int ncand = sel ? K : (int)M;

  // 2. one ordered sweep, a contiguous run of quads per thread: keys above tkey are appended in any order (ranked below), the ties
  //    at tkey take the slots behind them in anchor order
  {
    const int chunk = (nq + DETW_THREADS - 1) / DETW_THREADS;
    const int lo = min(nq, tid * chunk), hi = min(nq, lo + chunk);
    unsigned r = 0u;
    if (sel) {
      unsigned c2 = 0u;
      for (int q = lo; q < hi; ++q) {
        u32x4_w v = ws4[q];
        if (DETW_PAD_ANY && q == nq - 1) { if (A4 - A > 2) v.y = 0u; if (A4 - A > 1) v.z = 0u; if (A4 - A > 0) v.w = 0u; }
        c2 += (v.x == tkey ? 1u : 0u) + (v.y == tkey ? 1u : 0u) + (v.z == tkey ? 1u : 0u) + (v.w == tkey ? 1u : 0u);
      }
      unsigned tot2;
      r = detw_excl_scan(c2, tot2, wave_tot, lane, wave);
    }
    for (int q = lo; q < hi; ++q) {
      u32x4_w v = ws4[q];
      if (DETW_PAD_ANY && q == nq - 1) { if (A4 - A > 2) v.y = 0u; if (A4 - A > 1) v.z = 0u; if (A4 - A > 0) v.w = 0u; }
      const unsigned ks[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned k = ks[e];
        const unsigned long long word = ((unsigned long long)k << 32) | (unsigned long long)(0xffffffffu - (unsigned)(4 * q + e));
        if (k > tkey) {
          const unsigned pos = atomicAdd(&sv[2], 1u);
          if (pos < n_gt) cand[pos] = word;
        } else if (sel && k == tkey && r < need) {
          cand[n_gt + r] = word; ++r;
        }
      }
    }
  }
  __syncthreads();

  // 3. rank: score descending, anchor index ascending = the 64-bit words descending; they are distinct, so the ranks are a permutation
  {
    unsigned long long mine = 0ull;
    int rank = 0;
    if (tid < ncand) {
      mine = cand[tid];
      for (int j = 0; j < ncand; ++j) rank += (cand[j] > mine) ? 1 : 0;
    }
    __syncthreads();
    if (tid < ncand) cand[rank] = mine;
    __syncthreads();
  }

  // 4. thread r decodes the candidate of rank r
  const bool ok = tid < ncand;
  float score = 0.f; int cls = -1, idx = 0;
  BoxF bx = {0.f, 0.f, 0.f, 0.f};
#ifdef DETW_VIEWS
  // the view-aware decode: candidate s belongs to view v = s / ceil4(A), row b * V + v of pred and of the view table; its box is
  // anchor_box's, mapped into image coordinates by detv_map BEFORE any IoU is taken; idx becomes the pooled index p = v * A + anchor
  if (MANY) {
    const int j = tid & (MC_LANES - 1);
    for (int r = tid / MC_LANES; r < ncand; r += DETW_THREADS / MC_LANES) {
      const int s = (int)(0xffffffffu - (unsigned)(cand[r] & 0xffffffffull));
      const int v = s / A4, ai = s - v * A4;
      const long long row = (long long)b * (DETW_VIEWS) + v;
      const float* p = a.pred + (row * A + ai) * (C + 5);
      float sc; int c;
      mc_anchor_score<MC_REGS>(p, C, j, sc, c);
      if (j == 0) {
        const BoxF bb = detv_map(anchor_box(p + C + 1, a.anchors + 4 * ai, a.wmax, a.hmax), (DETW_VIEW_XF) + 6 * row);
        boxL[r] = (f32x4){bb.x1, bb.y1, bb.x2, bb.y2};
        clsL[r] = c;
      }
    }
    __syncthreads();
    if (ok) {
      const int s = (int)(0xffffffffu - (unsigned)(cand[tid] & 0xffffffffull));
      const int v = s / A4;
      idx = v * A + (s - v * A4);
      score = __uint_as_float((unsigned)(cand[tid] >> 32));
      cls = clsL[tid];
      const f32x4 bv = boxL[tid];
      bx.x1 = bv.x; bx.y1 = bv.y; bx.x2 = bv.z; bx.y2 = bv.w;
    }
  } else if (ok) {
    const int s = (int)(0xffffffffu - (unsigned)(cand[tid] & 0xffffffffull));
    const int v = s / A4, ai = s - v * A4;
    const long long row = (long long)b * (DETW_VIEWS) + v;
    const float* p = a.pred + (row * A + ai) * (C + 5);
    idx = v * A + ai;
    anchor_score(p, C, score, cls);
    bx = detv_map(anchor_box(p + C + 1, a.anchors + 4 * ai, a.wmax, a.hmax), (DETW_VIEW_XF) + 6 * row);
    boxL[tid] = (f32x4){bx.x1, bx.y1, bx.x2, bx.y2};
    clsL[tid] = cls;
  }
#else
  if (MANY && !dense) {
    // a 16-lane group per candidate (64 groups, <= 16 rounds): the class comes from the same mc_anchor_score that made the key, so
    // the score IS the key; lane 0 of the group decodes the box
    const int j = tid & (MC_LANES - 1);
    for (int r = tid / MC_LANES; r < ncand; r += DETW_THREADS / MC_LANES) {
      const int ai = (int)(0xffffffffu - (unsigned)(cand[r] & 0xffffffffull));
      const float* p = a.pred + ((long long)b * A + ai) * (C + 5);
      float s; int c;
      mc_anchor_score<MC_REGS>(p, C, j, s, c);
      if (j == 0) {
        const BoxF bb = anchor_box(p + C + 1, a.anchors + 4 * ai, a.wmax, a.hmax);
        boxL[r] = (f32x4){bb.x1, bb.y1, bb.x2, bb.y2};
        clsL[r] = c;
      }
    }
    __syncthreads();
    if (ok) {
      idx = (int)(0xffffffffu - (unsigned)(cand[tid] & 0xffffffffull));
      score = __uint_as_float((unsigned)(cand[tid] >> 32));
      cls = clsL[tid];
      const f32x4 v = boxL[tid];
      bx.x1 = v.x; bx.y1 = v.y; bx.x2 = v.z; bx.y2 = v.w;
    }
  } else if (ok) {
    idx = (int)(0xffffffffu - (unsigned)(cand[tid] & 0xffffffffull));
    if (dense) {
      const long long o = (long long)b * A + idx;
      score = a.in_score[o]; cls = (int)a.in_class[o];
      const f32x4 v = *(const f32x4*)(a.in_box + 4 * o);
      bx.x1 = v.x; bx.y1 = v.y; bx.x2 = v.z; bx.y2 = v.w;
    } else {
      const float* p = a.pred + ((long long)b * A + idx) * (C + 5);
      anchor_score(p, C, score, cls);
      bx = anchor_box(p + C + 1, a.anchors + 4 * idx, a.wmax, a.hmax);
    }
    boxL[tid] = (f32x4){bx.x1, bx.y1, bx.x2, bx.y2};
    clsL[tid] = cls;
  }
#endif
  __syncthreads();
