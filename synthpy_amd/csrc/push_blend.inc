// What k_push (push.hip) and k_push_matter (push_matter.hip) share of a step: a vector field's corner rows and their blend, and
// |a|^2 in the order include/synthray.h fixes.  Included inside each file's unnamed namespace.
template <typename T>
struct Row {  // one corner row: nodes k, k + 1 of z, three components each
  T v[6];
};

// the three components of one field at the cell (ci, cj, ck) with the blend of sr_field_resample's rule
template <typename T>
__device__ __forceinline__ void blend(const T *__restrict__ src, int64_t sx, int64_t sy, int ci, int cj, int ck, double ux, double wx,
                                      double w00, double w01, double w10, double w11, double (&val)[3]) {
  const T *p = src + ((int64_t)ci * sx + (int64_t)cj * sy + (int64_t)ck * 3);
  const Row<T> a0 = *reinterpret_cast<const Row<T> *>(p), a1 = *reinterpret_cast<const Row<T> *>(p + sy);
  const Row<T> b0 = *reinterpret_cast<const Row<T> *>(p + sx), b1 = *reinterpret_cast<const Row<T> *>(p + sx + sy);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s0 = (((double)a0.v[c] * w00 + (double)a0.v[3 + c] * w01) + (double)a1.v[c] * w10) + (double)a1.v[3 + c] * w11;
    const double s1 = (((double)b0.v[c] * w00 + (double)b0.v[3 + c] * w01) + (double)b1.v[c] * w10) + (double)b1.v[3 + c] * w11;
    val[c] = ux * s0 + wx * s1;
  }
}

__device__ __forceinline__ double norm2(double a0, double a1, double a2) { return (a0 * a0 + a1 * a1) + a2 * a2; }
