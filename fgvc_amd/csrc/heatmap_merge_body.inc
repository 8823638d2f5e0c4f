// The body of heatmap_merge_kernel (PEAK false) and heatmap_peak_merge_kernel (PEAK true; `peak` [K][T]), included into both so that the first
// stays the kernel it was, instruction for instruction: one thread per (frame, joint) map merges its bands and writes the coordinates; PEAK:
// also the largest of the map's values, the first of its top five, to peak[k][f].
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= T * K) return;
  const int f = m / K, k = m - f * K;
  Top5 top;
  top.init();
  double sum = 0.0;
  for (int b = 0; b < nbands; ++b) {
    const size_t o = (size_t)m * nbands + b;
    sum += part_sum[o];
    for (int j = 0; j < HM_K; ++j) {
      const int id = part_i[o * HM_K + j];
      const double v = part_v[o * HM_K + j];
      if (id >= 0 && top.accepts(v, id)) top.insert(v, id);
    }
  }
  double* ox = coords + (size_t)k * T + f;
  double* oy = ox + (size_t)K * T;
  if (PEAK) peak[(size_t)k * T + f] = top.v[0];
  if (sum == 0.0) {   // np.sum(map) == 0 (:189)
    *ox = -1.0;
    *oy = -1.0;
    return;
  }
  double ax = 0.0, ay = 0.0;
  if (f64) {
    double tot = 0.0;
#pragma unroll
    for (int j = HM_K - 1; j >= 0; --j) tot += top.v[j];
    tot += 1e-9;
#pragma unroll
    for (int j = HM_K - 1; j >= 0; --j) {
      const double wgt = top.v[j] / tot;
      ax += (double)(top.ix[j] % w0) * wgt;
      ay += (double)(top.ix[j] / w0) * wgt;
    }
  } else {
    float tot = 0.f;
#pragma unroll
    for (int j = HM_K - 1; j >= 0; --j) tot += (float)top.v[j];
    tot += 1e-9f;
#pragma unroll
    for (int j = HM_K - 1; j >= 0; --j) {
      const float wgt = (float)top.v[j] / tot;
      ax += (double)(top.ix[j] % w0) * (double)wgt;
      ay += (double)(top.ix[j] / w0) * (double)wgt;
    }
  }
  *ox = ax;
  *oy = ay;
