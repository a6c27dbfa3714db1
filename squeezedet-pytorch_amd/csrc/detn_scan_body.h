// Steps 5-7 of an NMS-modes select launch, as text: the (group, rank) order, the sequential scan of DESIGN.md section 3 "NMS modes" and
// the placement.  Included -- not called -- behind detw_select_body.h by detect_nms_select_kernel and by detect_views_select_kernel
// (pooled views: the same scan on image-coordinate boxes), for the reason given there: the text is what detect_nms_select_kernel
// always held, so its device code stays what it was.  The including kernel provides what detw_select_body.h left in scope, `n`
// (NmsArgs), the LDS arrays boxP, grpL, curL, outS, emitL [Kp], gstart, glen, gcnt, goff [256], slot_s, slot_p [2][16] and the macro
// DETN_STORE(pos, sc): store this thread's candidate as row `pos` of its image with the score `sc`.
// DETN_VOTE (off for those two kernels; the voting kernels define it as their VoteArgs): DESIGN.md section 3 "Box voting" -- between the
// scan and the store the thread of every emitted candidate replaces `bx` by the voted box (detn_vote) and writes its voter count.
  const int G = n.agnostic ? 1 : C;
  const float thr = a.score_thresh;

  // 5. order by (group, rank): slot = candidates of earlier groups + earlier ranks of my group
  const int g = (ok && cls >= 0 && cls < C) ? (n.agnostic ? 0 : cls) : -1;
  if (tid < Kp) { grpL[tid] = g; curL[tid] = -1.f; emitL[tid] = -1; }
  if (tid < 256) { glen[tid] = 0; gstart[tid] = 0; gcnt[tid] = 0u; }
  __syncthreads();
  int slot = 0;
  if (n.agnostic) {
    unsigned tot;
    slot = (int)detw_excl_scan(g >= 0 ? 1u : 0u, tot, wave_tot, lane, wave);
    if (tid == 0) glen[0] = (int)tot;
  } else if (g >= 0) {
    int before = 0, same_before = 0, same = 0;
    for (int r = 0; r < ncand; ++r) {
      const int gr = grpL[r];
      before += (gr >= 0 && (gr < g || (gr == g && r < tid))) ? 1 : 0;
      same_before += (gr == g && r < tid) ? 1 : 0;
      same += (gr == g) ? 1 : 0;
    }
    slot = before;
    if (same_before == 0) { gstart[g] = before; glen[g] = same; }
  }
  if (g >= 0) { boxP[slot] = (f32x4){bx.x1, bx.y1, bx.x2, bx.y2}; curL[slot] = score; }     // slot < ncand <= Kp
  __syncthreads();

  // 6. the scan
  if (n.agnostic && glen[0] > 64) {
    // one group on the whole workgroup: slot p in thread p's registers (glen[0] <= ncand <= 1024 = the threads)
    const int len = glen[0];
    const f32x4 me = boxP[tid < len ? tid : 0];
    float cur = tid < len ? curL[tid] : -1.f;
    int t = 0;
    for (;; ++t) {                                             // <= len + 1 rounds: every round but the last retires one candidate
      const float wm = nms_wave_max(cur);
      const unsigned long long hit = __ballot(cur == wm);
      float* ss = slot_s + 16 * (t & 1); int* sp = slot_p + 16 * (t & 1);
      if (lane == 0) { ss[wave] = wm; sp[wave] = hit ? wave * 64 + (__ffsll((long long)hit) - 1) : 0; }
      __syncthreads();
      const float v = lane < 16 ? ss[lane] : -1.f;
      const float m = nms_wave_max(v);
      if (!(m > thr)) break;                                   // (the same m in every wave: the whole workgroup leaves together)
      const unsigned long long wh = __ballot(lane < 16 && v == m);          // != 0: m is one of the v
      const int pp = sp[__ffsll((long long)wh) - 1];           // lowest wave = lowest slot = lowest rank
      const f32x4 pk = boxP[pp];
      const float pa = (pk.z - pk.x) * (pk.w - pk.y);
      if (tid == pp) { emitL[tid] = t; outS[tid] = m; cur = -1.f; }
      else if (cur >= 0.f) cur = nms_decay(n, a.nms_thresh, pk, pa, me, cur);
    }
    if (tid == 0) gcnt[0] = (unsigned)t;
  } else {
    for (int gi = wave; gi < G; gi += DETW_THREADS / 64) {
      const int s0 = gstart[gi], len = glen[gi];
      int t = 0;
      if (len <= 64) {
        const bool in = lane < len;
        const f32x4 me = boxP[in ? s0 + lane : 0];
        float cur = in ? curL[s0 + lane] : -1.f;
        for (; t < len; ++t) {
          const float m = nms_wave_max(cur);
          if (!(m > thr)) break;
          const int pl = __ffsll((long long)__ballot(cur == m)) - 1;        // (m > thr >= ... is one of the cur: the ballot is not empty)
          const f32x4 pk = boxP[s0 + pl];
          const float pa = (pk.z - pk.x) * (pk.w - pk.y);
          if (lane == pl) { emitL[s0 + lane] = t; outS[s0 + lane] = m; cur = -1.f; }
          else if (cur >= 0.f) cur = nms_decay(n, a.nms_thresh, pk, pa, me, cur);
        }
      } else {
        // the group strides over the lanes: slot s0 + lane + 64 i belongs to this lane alone, so curL needs no ordering between lanes
        float lm = -1.f; int lp = 0x7fffffff;
        for (int p = s0 + lane; p < s0 + len; p += 64) { const float c = curL[p]; if (c > lm) { lm = c; lp = p; } }
        for (; t < len; ++t) {
          const float m = nms_wave_max(lm);
          if (!(m > thr)) break;
          const int pp = nms_wave_min(lm == m ? lp : 0x7fffffff);           // lowest slot among the ties
          const f32x4 pk = boxP[pp];
          const float pa = (pk.z - pk.x) * (pk.w - pk.y);
          lm = -1.f; lp = 0x7fffffff;
          for (int p = s0 + lane; p < s0 + len; p += 64) {
            float c = curL[p];
            if (p == pp) { emitL[p] = t; outS[p] = m; c = -1.f; curL[p] = c; }
            else if (c >= 0.f) { c = nms_decay(n, a.nms_thresh, pk, pa, boxP[p], c); curL[p] = c; }
            if (c > lm) { lm = c; lp = p; }
          }
        }
      }
      if (lane == 0) gcnt[gi] = (unsigned)t;
    }
  }
  __syncthreads();

  // 7. placement: rows of the earlier groups + pick order
  {
    unsigned total;
    const unsigned off = detw_excl_scan((tid < G) ? gcnt[tid & 255] : 0u, total, wave_tot, lane, wave);
    if (tid < 256) goff[tid] = off;
    if (tid == 0) a.det_count[b] = (int)total;
  }
  __syncthreads();
  if (g >= 0) {
    const int t = emitL[slot];
#ifdef DETN_VOTE
    // box voting (the voting kernels define DETN_VOTE as their VoteArgs): the scan above is done and wrote none of cand / boxL / clsL,
    // so the thread of an emitted candidate replaces its box by the score-weighted mean of its cluster before the same store
    if (t >= 0) {
      const int nv = detn_vote(cand, boxL, clsL, ncand, tid, cls, (DETN_VOTE).iou, bx);
      if ((DETN_VOTE).votes) (DETN_VOTE).votes[(long long)b * K + (goff[g] + (unsigned)t)] = nv;
    }
#endif
    if (t >= 0) DETN_STORE(goff[g] + (unsigned)t, outS[slot]);
  }
