// Dynamic-time-warping score of a rollout against the reference motion, on the device: the
// evaluation metric of an imitate_amp run ('dtw_cost', milo/milo/utils.py:129-130 ->
// gym_deepmimic.py:160-162 -> cSceneImitateAMP::CalcRewardTimeWarp, DeepMimicCore/scenes/
// SceneImitateAMP.cpp:243-272).  This file restates cDynamicTimeWarper (DeepMimicCore/util/
// DynamicTimeWarper.cpp) quirks included, with either of its two cell costs:
//
//   val, AMX_DTW_COST_POINTS     cSceneImitateAMP::TimeWarpCost (SceneImitateAMP.cpp:5-25), the cost
//                                the scene's warper is built with (BuildTimeWarper, :510): the rows
//                                as dim / 3 points, the mean over the points of the Euclidean
//                                distance, sum_p sqrt(dx^2 + dy^2 + dz^2) / (dim / 3), summed in
//                                point order.  This is the cost of the reported 'dtw_cost'.
//   val, AMX_DTW_COST_SQUARED    cDynamicTimeWarper::DefaultCost (DynamicTimeWarper.cpp:3-8), what
//                                a warper initialised without a cost function uses:
//                                |data0[i] - data1[j]|^2 summed in index order.
//   CalcAlignment (:119-146)     C(0,0) = 0, the rest of row 0 / column 0 +inf;
//                                C(i,j) = val(i,j) + min(C(i-1,j-1), min(C(i-1,j), C(i,j-1))) for
//                                i, j >= 1: sample 0 of either side is never scored.
//                                Cost = C(n-1, m-1).
//   CalcIndexBuffer (:148-200)   backtrack from (n-1, m-1): diagonal when cost0 <= cost1 &&
//                                cost0 <= cost2, else up when cost1 <= cost2, else left; a left move
//                                accumulates the running cost, a diagonal / up move writes
//                                backtrack[i] and clears it; index[i] = j on every visit; the rows
//                                [0, i] left when the walk ends get index 0 and backtrack 0 (the
//                                reference's self-cost of a sample).
//   AddRemainderCost (:202-214)  backtrack += backtrack / sum(backtrack) * remainder, remainder =
//                                (buffer_size - n) * 1.0 (SceneImitateAMP.cpp:263-268); an all-zero
//                                backtrack becomes NaN there, and does here.  (Eigen's sum() and
//                                norm() associate their terms as its vectorisation decides; here
//                                both run in index order.  On exactly summable data they agree.)
//
// One 512-thread workgroup per trajectory (so n_max <= 513), three phases in one launch:
//   1. val(i,j) for every i, j >= 1 into the trajectory's n_max x n_max cost buffer (global
//      workspace): 32 x 64 tiles, both row blocks staged in LDS, four cells per thread.
//   2. the recurrence, one anti-diagonal per barrier (cells of a diagonal are independent): thread
//      k owns row i = k + 1 and walks it left to right, so the val cells it needs are contiguous:
//      it loads the next eight of them at once every eighth diagonal (one exposed memory latency
//      per eight barriers, not one per barrier), takes the three predecessors from the previous
//      two diagonals kept in LDS (three rotating n_max buffers), and writes the cost back to the
//      cell and to the current LDS diagonal.  n + m - 3 barriers.
//   3. lane 0 walks the backtrack (<= n + m steps; every step lowers i or j, so it ends whatever
//      the data), filling index / backtrack in LDS; the workgroup then applies the remainder and
//      writes the outputs.
// The cost buffer stays in global memory because the backtrack reads cost differences anywhere
// along the path (730 KB per trajectory at 302; a CU has 160 KiB of LDS).  LDS per workgroup:
// (3 n_max + 96 dim) doubles = 42 KB at n_max 302, dim 45, so three workgroups fit a CU.  Every
// global word a workgroup reads back was written by the same workgroup before a barrier.
// fp64 throughout; contraction is off for the file, so val, the recurrence and the remainder
// round like the reference's separate IEEE operations.
#include "amx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 512;            // threads per workgroup: thread k owns row k + 1 of the cost buffer
constexpr int TI = 32, TJ = 64;    // val tile: rows of data0 (four per wave) x rows of data1 (one per lane)
constexpr int CH = 8;              // diagonals per val prefetch
constexpr long long LDS_MAX = 65536;

__host__ __device__ inline long long dtw_lds_bytes(int n_max, int dim) {
  return (3LL * n_max + (long long)(TI + TJ) * dim) * (long long)sizeof(double);
}

__global__ __launch_bounds__(NT) void k_dtw_align(const double* __restrict__ data0, const double* __restrict__ data1,
                                                  long long ld, int dim, int cost_kind, int n_max,
                                                  const int32_t* __restrict__ len, int buffer_size, double* work, double* __restrict__ cost,
                                                  double* __restrict__ dtw_cost, int32_t* __restrict__ index,
                                                  double* __restrict__ bt_raw, double* __restrict__ bt_out) {
  extern __shared__ double lds[];
  double* diag = lds;                 // [3][n_max]
  double* a = diag + 3 * n_max;       // [TI][dim]
  double* b = a + TI * dim;           // [TJ][dim]
  const int t = blockIdx.x, tid = threadIdx.x;
  int n = len[t];
  n = n < 2 ? 2 : (n > n_max ? n_max : n);   // validated on the host; never index past the buffers
  const double* d0 = data0 + (long long)t * n_max * ld;
  const double* d1 = data1 + (long long)t * n_max * ld;
  double* C = work + (long long)t * n_max * n_max;
  const double inf = __builtin_huge_val();

  // ---- borders and val ---------------------------------------------------------------------------
  for (int k = tid; k < n; k += NT) {
    const double v = k == 0 ? 0.0 : inf;
    C[k] = v;
    C[(long long)k * n_max] = v;
  }
  const int w = tid >> 6, lane = tid & 63;
  for (int j0 = 1; j0 < n; j0 += TJ) {
    __syncthreads();
    for (int e = tid; e < TJ * dim; e += NT) {
      const int r = j0 + e / dim;
      b[e] = r < n ? d1[(long long)r * ld + e % dim] : 0.0;
    }
    for (int i0 = 1; i0 < n; i0 += TI) {
      __syncthreads();
      for (int e = tid; e < TI * dim; e += NT) {
        const int r = i0 + e / dim;
        a[e] = r < n ? d0[(long long)r * ld + e % dim] : 0.0;
      }
      __syncthreads();
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const double* br = b + lane * dim;
      const double* ar = a + (w * 4) * dim;
      if (cost_kind == AMX_DTW_COST_SQUARED) {
        for (int k = 0; k < dim; ++k) {
          const double bv = br[k];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double d = ar[r * dim + k] - bv;
            acc[r] = acc[r] + d * d;
          }
        }
      } else {   // TimeWarpCost: mean point distance (dim % 3 == 0, checked on the host)
        const int np = dim / 3;
        for (int p = 0; p < np; ++p) {
          const double bx = br[3 * p], by = br[3 * p + 1], bz = br[3 * p + 2];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double* q = ar + r * dim + 3 * p;   // pt1 - pt0 with pt0 = data0's, pt1 = data1's
            const double dx = bx - q[0], dy = by - q[1], dz = bz - q[2];
            acc[r] = acc[r] + sqrt(dx * dx + dy * dy + dz * dz);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] / (double)np;
      }
      const int j = j0 + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + w * 4 + r;
        if (i < n && j < n) C[(long long)i * n_max + j] = acc[r];
      }
    }
  }
  __syncthreads();

  // ---- the recurrence, one anti-diagonal d = i + j per barrier -----------------------------------
  const int ri = tid + 1;                     // this thread's row (idle when ri >= n)
  double* row = C + (long long)(ri < n ? ri : 0) * n_max;
  const int dmax = 2 * (n - 1);
  for (int d0 = 2; d0 <= dmax; d0 += CH) {
    double v[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {            // val of this row's cells on diagonals d0 .. d0 + CH - 1
      const int j = d0 + c - ri;
      v[c] = (ri < n && j >= 1 && j < n) ? row[j] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int d = d0 + c;
      if (d > dmax) break;                    // (uniform over the workgroup)
      double* cur = diag + (d % 3) * n_max;
      const double* p1 = diag + ((d + 2) % 3) * n_max;   // diagonal d - 1, by row
      const double* p2 = diag + ((d + 1) % 3) * n_max;   // diagonal d - 2
      const int j = d - ri;
      if (ri < n && j >= 1 && j < n) {
        const double cost0 = (ri == 1 && j == 1) ? 0.0 : ((ri == 1 || j == 1) ? inf : p2[ri - 1]);
        const double cost1 = ri == 1 ? inf : p1[ri - 1];
        const double cost2 = j == 1 ? inf : p1[ri];
        const double m12 = cost2 < cost1 ? cost2 : cost1;   // std::min(cost1, cost2)
        const double mn = m12 < cost0 ? m12 : cost0;        // std::min(cost0, .)
        const double cst = v[c] + mn;
        cur[ri] = cst;
        row[j] = cst;
      }
      __syncthreads();
    }
  }

  // ---- backtrack (one lane), remainder, outputs --------------------------------------------------
  double* bt = diag;                                   // [n_max]
  int32_t* idx = (int32_t*)(diag + n_max);             // [n_max]
  double* s_sum = diag + 2 * n_max;                    // sum(backtrack)
  if (tid == 0) {
    int i = n - 1, j = n - 1;
    double run = 0.0;
    double total = C[(long long)i * n_max + j];
    while (i >= 1 && j >= 1) {
      idx[i] = j;
      const double cost0 = C[(long long)(i - 1) * n_max + j - 1];
      const double cost1 = C[(long long)(i - 1) * n_max + j];
      const double cost2 = C[(long long)i * n_max + j - 1];
      if (cost0 <= cost1 && cost0 <= cost2) {
        run += total - cost0;
        bt[i] = run;
        run = 0.0;
        --i; --j;
        total = cost0;
      } else if (cost1 <= cost2) {
        run += total - cost1;
        bt[i] = run;
        run = 0.0;
        --i;
        total = cost1;
      } else {
        run += total - cost2;
        --j;
        total = cost2;
      }
    }
    for (int k = 0; k <= i; ++k) {
      idx[k] = 0;
      bt[k] = 0.0;
    }
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += bt[k];
    *s_sum = s;
    const double align = C[(long long)(n - 1) * n_max + (n - 1)];
    const double rem = (double)(buffer_size - n) * 1.0;
    cost[t] = align;
    if (dtw_cost) dtw_cost[t] = align + rem;
  }
  __syncthreads();
  const double rem = (double)(buffer_size - n) * 1.0;
  const double sum = *s_sum;
  for (int k = tid; k < n; k += NT) {
    const double raw = bt[k];
    const long long o = (long long)t * n_max + k;
    index[o] = idx[k];
    if (bt_raw) bt_raw[o] = raw;
    const double share = raw / sum;
    bt_out[o] = raw + share * rem;
  }
}

}  // namespace

extern "C" long long amx_dtw_work(int T, int n_max) {
  if (T < 0 || n_max < 2) return -1;
  return (long long)T * n_max * n_max;
}

extern "C" int amx_dtw_align(amx_ctx* c, const double* data0, const double* data1, long long ld, int dim, int cost_kind,
                             int n_max,
                             const int32_t* len_host, const int32_t* len, int T, int buffer_size, double* work,
                             double* cost, double* dtw_cost, int32_t* index, double* backtrack_raw,
                             double* backtrack, void* stream) {
  AMX_CHECK_ARG(c, "amx_dtw_align: null context");
  AMX_CHECK_ARG(data0 && data1 && len_host && len && work && cost && index && backtrack,
                "amx_dtw_align: null pointer");
  AMX_CHECK_ARG(T >= 0 && dim >= 1 && n_max >= 2 && n_max <= NT + 1, "amx_dtw_align: T=%d dim=%d n_max=%d (2..%d)", T,
                dim, n_max, NT + 1);
  AMX_CHECK_ARG(ld >= dim, "amx_dtw_align: ld=%lld < dim=%d", ld, dim);
  AMX_CHECK_ARG(cost_kind == AMX_DTW_COST_SQUARED || (cost_kind == AMX_DTW_COST_POINTS && dim % 3 == 0),
                "amx_dtw_align: cost=%d with dim=%d (AMX_DTW_COST_POINTS needs rows of 3-d points)", cost_kind, dim);
  AMX_CHECK_ARG(dtw_lds_bytes(n_max, dim) <= LDS_MAX,
                "amx_dtw_align: n_max=%d, dim=%d need %lld bytes of LDS (most %lld)", n_max, dim,
                dtw_lds_bytes(n_max, dim), LDS_MAX);
  for (int t = 0; t < T; ++t) {
    AMX_CHECK_ARG(len_host[t] >= 2 && len_host[t] <= n_max, "amx_dtw_align: len[%d]=%d outside [2, n_max=%d]", t,
                  len_host[t], n_max);
    AMX_CHECK_ARG(buffer_size >= len_host[t], "amx_dtw_align: buffer_size=%d < len[%d]=%d", buffer_size, t,
                  len_host[t]);
  }
  if (T == 0) return AMX_OK;
  hipLaunchKernelGGL(k_dtw_align, dim3(T), dim3(NT), (size_t)dtw_lds_bytes(n_max, dim), (hipStream_t)stream, data0,
                     data1, ld, dim, cost_kind, n_max, len, buffer_size, work, cost, dtw_cost, index, backtrack_raw, backtrack);
  AMX_CHECK_LAUNCH();
  return AMX_OK;
}
