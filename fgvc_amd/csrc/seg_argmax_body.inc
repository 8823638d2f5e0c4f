// The body of read-out phase 2, included by seg_argmax_kernel (CONF = false) and seg_readout_conf_kernel (CONF = true) in seg.hip: one text,
// so the two cannot drift apart, and the first kernel compiles to the instructions it had before the second existed.  In scope: labels, g,
// part, norm, masks, `extra` (SegConfOut: read under CONF only), the template parameter COMPOSED and the constant CONF.
  extern __shared__ float mm[];  // [C][2]: min, max (CONF: | cnt[C] | sum[C])
  const int f = blockIdx.y, C = g.C;
  const int HW = g.h0 * g.w0;
  const float* lab = labels + (size_t)f * g.Hf * g.Wf * C;
  const float* src = part + (size_t)f * SEG_NB * C * 2;
  for (int c = threadIdx.x; c < C; c += SEG_BLOCK) {
    float mn = INFINITY, mx = -INFINITY;
    for (int b = 0; b < SEG_NB; ++b) {
      mn = fminf(mn, src[(b * C + c) * 2]);
      mx = fmaxf(mx, src[(b * C + c) * 2 + 1]);
    }
    mm[2 * c] = mn;
    mm[2 * c + 1] = mx;
  }
  if constexpr (CONF) {
    uint32_t* cnt = reinterpret_cast<uint32_t*>(mm + 2 * C);
    for (int c = threadIdx.x; c < 2 * C; c += SEG_BLOCK) cnt[c] = 0u;
  }
  __syncthreads();
  const int p = blockIdx.x * SEG_CHUNK + threadIdx.x * SEG_PX;
  if constexpr (!CONF) {
    if (p >= HW) return;
  }
  if (CONF ? p < HW : true) {   // (the block keeps the indentation of the lines it wraps)
  Taps<COMPOSED> ty[SEG_PX], tx[SEG_PX];
  lane_taps<COMPOSED>(g, p, HW, ty, tx);
  float best[SEG_PX], second[CONF ? SEG_PX : 1];
  int bi[SEG_PX];
#pragma unroll
  for (int k = 0; k < SEG_PX; ++k) {
    best[k] = -INFINITY;
    if constexpr (CONF) second[k] = -INFINITY;
    bi[k] = 0;
  }
  for (int c = 0; c < C; ++c) {
    const float mn = mm[2 * c], mx = mm[2 * c + 1];
    // torch.where(max > 0, (x - min) / (max - min + 1e-12), x)
    const bool nrm = norm && mx > 0.f;
    const float den = (mx - mn) + 1e-12f;
#pragma unroll
    for (int k = 0; k < SEG_PX; ++k) {
      float v = field_value<COMPOSED>(lab + c, ty[k], tx[k]);
      if (nrm) v = (v - mn) / den;
      if constexpr (CONF) second[k] = (c == 0 || v > best[k]) ? best[k] : fmaxf(second[k], v);
      if (c == 0 || v > best[k]) {
        best[k] = v;
        bi[k] = c;
      }
    }
  }
  uint8_t* dst = masks + (size_t)f * HW + p;
  if (p + SEG_PX <= HW && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    const uint32_t word = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
    *reinterpret_cast<uint32_t*>(dst) = word;
  } else {
#pragma unroll
    for (int k = 0; k < SEG_PX; ++k)
      if (p + k < HW) dst[k] = (uint8_t)bi[k];
  }
  if constexpr (CONF) {
    uint32_t* cnt = reinterpret_cast<uint32_t*>(mm + 2 * C);
    uint32_t cb[SEG_PX];
#pragma unroll
    for (int k = 0; k < SEG_PX; ++k) {
      const float gap = fminf(fmaxf(best[k] - second[k], 0.f), 1.f);
      cb[k] = (uint32_t)rintf(255.f * gap);
      if (p + k < HW) {
        atomicAdd(&cnt[bi[k]], 1u);
        atomicAdd(&cnt[C + bi[k]], cb[k]);
      }
    }
    uint8_t* dc = extra.conf + (size_t)f * HW + p;
    if (p + SEG_PX <= HW && (reinterpret_cast<uintptr_t>(dc) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(dc) = cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < SEG_PX; ++k)
        if (p + k < HW) dc[k] = (uint8_t)cb[k];
    }
  }
  }
  if constexpr (CONF) {
    uint32_t* cnt = reinterpret_cast<uint32_t*>(mm + 2 * C);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += SEG_BLOCK)
      if (cnt[c] != 0u) {
        unsigned long long* dst = extra.stats + ((size_t)f * C + c) * 2;
        atomicAdd(dst, (unsigned long long)cnt[c]);
        atomicAdd(dst + 1, (unsigned long long)cnt[C + c]);
      }
  }
