// ocs_matlab.hpp -- private, host only: the MATLAB-semantics helpers the C-ABI translation units share (ocs_control.cpp,
// ocs_fbs.cpp).  One definition each, so that every table built from them is the same to the last bit.
#pragma once

namespace ocs {

// linspace(d1, d2, n):  d1 + (0:n1).*(d2-d1)./n1 with the end points pinned
inline void matlab_linspace(double a, double b, int n, double* out) {
  if (n <= 0) return;
  if (n == 1) {
    out[0] = b;
    return;
  }
  const int n1 = n - 1;
  for (int k = 0; k <= n1; ++k) out[k] = a + ((double)k * (b - a)) / (double)n1;
  out[0] = a;
  out[n1] = b;
}

// the interval of the sorted grid x[0..n) a query lies in: k with x[k] <= q < x[k+1], 0 before the grid, n - 2 from its end on
inline int interval_of(int n, const double* x, double q) {
  if (q <= x[0]) return 0;
  if (q >= x[n - 1]) return n - 2;
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (x[mid] <= q)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// pchip weights of the node between two intervals of lengths hl, hr (MATLAB pchipslopes)
inline void pchip_weight_pair(double hl, double hr, double* w1, double* w2) {
  const double hs = hl + hr;
  *w1 = (hl + hs) / (3 * hs);
  *w2 = (hs + hr) / (3 * hs);
}
// ... of every interior node of a grid of n nodes with interval lengths h[0..n-1); the end nodes get 0
inline void pchip_weights(int n, const double* h, double* w1, double* w2) {
  for (int k = 0; k < n; ++k) w1[k] = w2[k] = 0.0;
  for (int k = 1; k + 1 < n; ++k) pchip_weight_pair(h[k - 1], h[k], &w1[k], &w2[k]);
}

}  // namespace ocs
