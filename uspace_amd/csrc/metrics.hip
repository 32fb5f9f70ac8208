// Feature-set metrics (KID, precision / recall / density / coverage, RBF-kernel MMD / CMMD, nearest neighbours): reductions over the pairwise
// quantities of two fp32 feature sets x [nx, F] and y [ny, F], computed in fp64 on v_mfma_f64_16x16x4_f64 and never stored as an nx x ny matrix.
//
// One tile engine, five consumers.  A workgroup (4 waves) owns 64 rows of x and walks every 128-column tile of y; wave w owns
// rows 16 w .. 16 w + 15 of the block against all 128 columns (8 MFMA tiles), so a row lives in ONE wave and every reduction along
// a row is finished inside it: integer adds and minima (exact in any order), or fp64 sums in one fixed order.  No atomics.
//   dot(i, j)  the fp64 MFMA over the fp32 values widened to fp64; k beyond F contributes exact zeros
//   D2(i, j) = max(0, fma(-2, dot, |x_i|^2 + |y_j|^2)), the squared norms from norms_kernel (one fixed order, so a norm has the same
//              bits wherever it is used)
// Operand tiles are staged through LDS as fp32 [row][32 + 4] by 16-byte loads (8 consecutive lanes read 128 contiguous bytes of a
// row), the next K step's loads in flight in registers while this one is multiplied.  A lane reads a float4 at k = 16 h + 4 g .. + 3
// (g = lane >> 4) and feeds component c to the c-th of four MFMAs: the MFMA's k index is then {16 h + 4 g + c : g}, a permutation
// of the K step that both operands share.  The row stride of 36 floats (144 B) puts the 16 rows of a fragment on 16 distinct 16-byte
// slots of the 256-byte bank row.
// Tile sizes, the single LDS buffer and the occupancy are a first choice: no alternative was measured.
#include "common.h"

#include <cfloat>
#include <climits>

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int kBM = 64;            // rows of x per workgroup
constexpr int kBN = 128;           // columns (rows of y) per tile
constexpr int kBK = 32;            // K step
constexpr int kLD = kBK + 4;       // LDS row stride in floats
constexpr int kNT = kBN / 16;      // MFMA tiles per wave along the columns
constexpr int kMaxK = 16;          // neighbours kept per row
constexpr int kMaxN = 1 << 24;

__device__ __forceinline__ double dist2(double nx, double ny, double dot) { return fmax(0.0, __fma_rn(-2.0, dot, nx + ny)); }

// |x_r|^2 in fp64: one wave per row, lane l sums k = l, l + 64, ... in order, then a fixed xor tree
__global__ __launch_bounds__(256) void norms_kernel(const float* __restrict__ x, int n, int F, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* p = x + (size_t)r * F;
    double s = 0.0;
    for (int k = lane; k < F; k += 64) {
        const double v = (double)p[k];
        s = __fma_rn(v, v, s);
    }
    s = wave_sum_f64(s);
    if (lane == 0) out[r] = s;
}

__device__ __forceinline__ float4 load4(const float* __restrict__ p, int k, int F, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!p || k >= F) return v;
    if (vec) return *reinterpret_cast<const float4*>(p + k);      // F % 4 == 0 and k % 4 == 0: k + 3 < F
    v.x = p[k];
    if (k + 1 < F) v.y = p[k + 1];
    if (k + 2 < F) v.z = p[k + 2];
    if (k + 3 < F) v.w = p[k + 3];
    return v;
}

// The engine.  C supplies: F, vec; n_cols(); row_a(r) / row_b(j): the fp32 row behind block-space index r / column j, or
// nullptr beyond the set (staged as zeros); init(scratch); tile(acc, col0, scratch); finish(scratch).  acc[t][reg] of lane
// (g = lane >> 4, c = lane & 15) is dot(row0 + 16 wave + g + 4 reg, col0 + 16 t + c).  scratch is kBM * kMaxK doubles of LDS, followed
// by C::kIdxInts ints where the consumer declares any (TopkConsumer: the index lists; 0 leaves the array what it was).
template <class C>
__global__ __launch_bounds__(256, 2) void gram_kernel(C c) {
    __shared__ __attribute__((aligned(16))) float As[kBM * kLD];
    __shared__ __attribute__((aligned(16))) float Bs[kBN * kLD];
    __shared__ double scratch[kBM * kMaxK + C::kIdxInts / 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.x * kBM;
    const int F = c.F;
    // staging: float4 id = tid + 256 i -> tile row id >> 3, k quad id & 7
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    const float* pa[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) pa[i] = c.row_a(row0 + srow + 32 * i);
    c.init(scratch);
    const int n_cols = c.n_cols();
    for (int col0 = 0; col0 < n_cols; col0 += kBN) {
        const float* pb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pb[i] = c.row_b(col0 + srow + 32 * i);
        f64x4 acc[kNT];
#pragma unroll
        for (int t = 0; t < kNT; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
        float4 ra[2], rb[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) ra[i] = load4(pa[i], sk, F, c.vec);
#pragma unroll
        for (int i = 0; i < 4; ++i) rb[i] = load4(pb[i], sk, F, c.vec);
        for (int k0 = 0; k0 < F; k0 += kBK) {
            __syncthreads();      // the previous step's (and the previous tile's consumer's) LDS reads are done
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&As[(srow + 32 * i) * kLD + sk]) = ra[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&Bs[(srow + 32 * i) * kLD + sk]) = rb[i];
            __syncthreads();
            if (k0 + kBK < F) {
#pragma unroll
                for (int i = 0; i < 2; ++i) ra[i] = load4(pa[i], k0 + kBK + sk, F, c.vec);
#pragma unroll
                for (int i = 0; i < 4; ++i) rb[i] = load4(pb[i], k0 + kBK + sk, F, c.vec);
            }
#pragma unroll
            for (int h = 0; h < kBK / 16; ++h) {
                const float4 a4 = *reinterpret_cast<const float4*>(&As[(wave * 16 + c16) * kLD + h * 16 + g * 4]);
                const double a[4] = {(double)a4.x, (double)a4.y, (double)a4.z, (double)a4.w};
#pragma unroll
                for (int t = 0; t < kNT; ++t) {
                    const float4 b4 = *reinterpret_cast<const float4*>(&Bs[(t * 16 + c16) * kLD + h * 16 + g * 4]);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], (double)b4.x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], (double)b4.y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2], (double)b4.z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[3], (double)b4.w, acc[t], 0, 0, 0);
                }
            }
        }
        c.tile(acc, col0, scratch);
    }
    c.finish(scratch);
}

// ---- consumer 1: the k smallest D2(i, j), j != i, of every row.  The row's sorted list lives in LDS (scratch[row][k]); a tile's
// candidates are compared with the list's last entry first, and only a wave that holds a smaller one takes the insertion path,
// the 16 lanes of a row one after the other in explicit turns (see tile()).  The kept multiset is the k smallest whatever
// the order of insertion.
struct KnnConsumer {
    static constexpr int kIdxInts = 0;
    const float* x;
    const double* norm;
    double* radius2;
    int n, F, k;
    bool vec;
    double nr[4];
    int grow[4];

    __device__ int n_cols() const { return n; }
    __device__ const float* row_a(int r) const { return r < n ? x + (size_t)r * F : nullptr; }
    __device__ const float* row_b(int j) const { return row_a(j); }
    __device__ void init(double* scratch) {
        for (int i = threadIdx.x; i < kBM * kMaxK; i += 256) scratch[i] = __builtin_inf();
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            grow[r] = blockIdx.x * kBM + wave * 16 + (lane >> 4) + 4 * r;
            nr[r] = grow[r] < n ? norm[grow[r]] : 0.0;
        }
        __syncthreads();
    }
    __device__ void tile(f64x4 (&acc)[kNT], int col0, double* scratch) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
        volatile double* list = scratch + (wave * 16 + g) * kMaxK;      // + 4 reg * kMaxK: the list of row g + 4 reg
        double thr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) thr[r] = list[4 * r * kMaxK + k - 1];
        bool pass = false;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int col = col0 + t * 16 + c16;
            const double ny = col < n ? norm[col] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = col < n && grow[r] < n && col != grow[r];
                const double d = valid ? dist2(nr[r], ny, acc[t][r]) : __builtin_inf();
                acc[t][r] = d;
                pass |= d < thr[r];
            }
        }
        if (!__any(pass)) return;
        // One lane of a row at a time: the 16 lanes that share a row's list take turns in a wave-uniform loop, and a turn ends with a
        // wavefront-scope fence and a wave barrier, so the next lane's reads of the list are ordered after this lane's writes by the
        // memory model, not by the accident that a wave issues its LDS operations in program order.  Lanes of different g work on
        // different rows' lists and share a turn.
#pragma unroll 1
        for (int s = 0; s < 16; ++s) {
            if (__ballot(c16 == s && pass) == 0) continue;       // wave-uniform: nobody holds a candidate in this turn
            if (c16 == s && pass) {
#pragma unroll
                for (int t = 0; t < kNT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double v = acc[t][r];
                        volatile double* L = list + 4 * r * kMaxK;
                        if (v < L[k - 1]) {
                            int i = k - 1;
                            while (i > 0) {
                                const double u = L[i - 1];
                                if (!(u > v)) break;
                                L[i] = u;
                                --i;
                            }
                            L[i] = v;
                        }
                    }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __device__ void finish(double* scratch) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if ((lane & 15) != 0) return;
        volatile double* list = scratch + (wave * 16 + (lane >> 4)) * kMaxK;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (grow[r] < n) radius2[grow[r]] = list[4 * r * kMaxK + k - 1];
    }
};

// ---- consumer 2: count[i] = #{j : D2(i, j) <= radius2_y[j]} and min_d2[i] = min_j D2(i, j)
struct ManifoldConsumer {
    static constexpr int kIdxInts = 0;
    const float *x, *y;
    const double *norm_x, *norm_y, *radius2_y;
    int* count;
    double* min_d2;
    int nx, ny, F;
    bool vec;
    double nr[4], mn[4];
    int grow[4], cnt[4];

    __device__ int n_cols() const { return ny; }
    __device__ const float* row_a(int r) const { return r < nx ? x + (size_t)r * F : nullptr; }
    __device__ const float* row_b(int j) const { return j < ny ? y + (size_t)j * F : nullptr; }
    __device__ void init(double*) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            grow[r] = blockIdx.x * kBM + wave * 16 + (lane >> 4) + 4 * r;
            nr[r] = grow[r] < nx ? norm_x[grow[r]] : 0.0;
            mn[r] = __builtin_inf();
            cnt[r] = 0;
        }
    }
    __device__ void tile(f64x4 (&acc)[kNT], int col0, double*) {
        const int c16 = threadIdx.x & 15;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int col = col0 + t * 16 + c16;
            if (col >= ny) continue;
            const double nyj = norm_y[col];
            const double r2 = radius2_y ? radius2_y[col] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double d = dist2(nr[r], nyj, acc[t][r]);
                mn[r] = fmin(mn[r], d);
                if (radius2_y) cnt[r] += d <= r2 ? 1 : 0;
            }
        }
    }
    __device__ void finish(double*) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {       // the 16 lanes of a row: lane ^ o keeps lane >> 4
                mn[r] = fmin(mn[r], __shfl_xor(mn[r], o, 64));
                cnt[r] += __shfl_xor(cnt[r], o, 64);
            }
            if ((threadIdx.x & 15) == 0 && grow[r] < nx) {
                if (count) count[grow[r]] = cnt[r];
                if (min_d2) min_d2[grow[r]] = mn[r];
            }
        }
    }
};

// ---- consumer 3: sums of K(a, b) = (gamma a.b + coef0)^degree over the m x m pairs of a subset.  blockIdx.y: subset, blockIdx.z:
// 0 x against x, 1 y against y (both without the positions p == q), 2 x against y.  Lane sums in tile order, a fixed xor tree per
// wave, the four waves in order -> partial[(subset * 3 + which) * row_blocks + blockIdx.x]; poly_finish_kernel adds the row blocks.
struct PolyConsumer {
    static constexpr int kIdxInts = 0;
    const float *x, *y;
    const int *idx_x, *idx_y;
    double* partial;
    int m, F, degree;
    double gamma, coef0;
    bool vec;
    double sum;
    int prow[4];

    __device__ int which() const { return blockIdx.z; }
    __device__ int n_cols() const { return m; }
    __device__ const float* row_a(int p) const {
        if (p >= m) return nullptr;
        return which() == 1 ? y + (size_t)idx_y[(size_t)blockIdx.y * m + p] * F : x + (size_t)idx_x[(size_t)blockIdx.y * m + p] * F;
    }
    __device__ const float* row_b(int q) const {
        if (q >= m) return nullptr;
        return which() == 0 ? x + (size_t)idx_x[(size_t)blockIdx.y * m + q] * F : y + (size_t)idx_y[(size_t)blockIdx.y * m + q] * F;
    }
    __device__ void init(double*) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        sum = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) prow[r] = blockIdx.x * kBM + wave * 16 + (lane >> 4) + 4 * r;
    }
    __device__ void tile(f64x4 (&acc)[kNT], int col0, double*) {
        const int c16 = threadIdx.x & 15;
        const bool off_diagonal_only = which() != 2;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int q = col0 + t * 16 + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = __fma_rn(gamma, acc[t][r], coef0);
                double pw = v;
                for (int d = 1; d < degree; ++d) pw *= v;
                if (q < m && prow[r] < m && !(off_diagonal_only && q == prow[r])) sum += pw;
            }
        }
    }
    __device__ void finish(double* scratch) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        sum = wave_sum_f64(sum);
        __syncthreads();
        if (lane == 0) scratch[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0)
            partial[((size_t)blockIdx.y * 3 + blockIdx.z) * gridDim.x + blockIdx.x] = ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
    }
};

// ---- consumer 4: sums of the Gaussian RBF kernel K(a, b) = exp(-gamma D2(a, b)) over whole sets.  blockIdx.z: 0 x against x,
// 1 y against y (both without i == j, left out by index), 2 x against y.  With `normalize` D2 is taken between a / |a| and
// b / |b|, formed in fp64 from the same dot and norms: dot * (1 / |a|)(1 / |b|) and squared norms of 1 (a zero row: factor and
// squared norm 0, the zero vector).  Without it the factors are 1 and the line below is dist2 of the raw values.  Elements
// beyond either set and the diagonal never enter the sum: a padded column has D2 = |a|^2 and K > 0, so it cannot be masked by
// value.  A row block beyond the pair's rows walks no tile and writes a zero partial.  Summation as PolyConsumer:
// partial[which * row_blocks + blockIdx.x], finished by poly_finish_kernel.
struct RbfConsumer {
    static constexpr int kIdxInts = 0;
    const float *x, *y;
    const double *norm_x, *norm_y;
    double* partial;
    int nx, ny, F;
    double gamma;
    bool normalize, vec;
    double sum;
    double na[4], sa[4];
    int prow[4];

    __device__ int which() const { return blockIdx.z; }
    __device__ int rows() const { return which() == 1 ? ny : nx; }
    __device__ int cols() const { return which() == 0 ? nx : ny; }
    __device__ int n_cols() const { return (int)blockIdx.x * kBM < rows() ? cols() : 0; }
    __device__ const float* row_a(int r) const { return r < rows() ? (which() == 1 ? y : x) + (size_t)r * F : nullptr; }
    __device__ const float* row_b(int j) const { return j < cols() ? (which() == 0 ? x : y) + (size_t)j * F : nullptr; }
    // (squared norm, factor on the dot product) of a row with squared norm n2
    __device__ void unit(double n2, double& n, double& s) const {
        if (!normalize) {
            n = n2;
            s = 1.0;
        } else {
            n = n2 > 0.0 ? 1.0 : 0.0;
            s = n2 > 0.0 ? 1.0 / sqrt(n2) : 0.0;
        }
    }
    __device__ void init(double*) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const double* norm_a = which() == 1 ? norm_y : norm_x;
        sum = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            prow[r] = blockIdx.x * kBM + wave * 16 + (lane >> 4) + 4 * r;
            unit(prow[r] < rows() ? norm_a[prow[r]] : 0.0, na[r], sa[r]);
        }
    }
    __device__ void tile(f64x4 (&acc)[kNT], int col0, double*) {
        const int c16 = threadIdx.x & 15;
        const bool off_diagonal_only = which() != 2;
        const double* norm_b = which() == 0 ? norm_x : norm_y;
        const int n_rows = rows(), n_col = cols();
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int q = col0 + t * 16 + c16;
            if (q >= n_col) continue;
            double nb, sb;
            unit(norm_b[q], nb, sb);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (prow[r] >= n_rows || (off_diagonal_only && q == prow[r])) continue;
                const double d = dist2(na[r], nb, acc[t][r] * (sa[r] * sb));
                sum += exp(-gamma * d);
            }
        }
    }
    __device__ void finish(double* scratch) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        sum = wave_sum_f64(sum);
        __syncthreads();
        if (lane == 0) scratch[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0)
            partial[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
    }
};

// ---- consumer 5: for every row i of x the k smallest D2(i, j) over the rows j of y WITH their indices: sorted lists of (d2, index)
// pairs per row in LDS, the distances in scratch[row][k] as KnnConsumer keeps them, the indices in the kIdxInts ints behind them.
// The order is lexicographic in (d2, global index), ascending, and the index comparison is written out in the insertion test: within
// one lane's turn the columns arrive as col0 + 16 t + c16, and the turns go through c16, so the walk order is not the index order.
// (The threshold test in front stays KnnConsumer's d < last: when a tile begins the list holds only earlier, hence smaller, columns,
// and whatever this tile inserts is smaller than that threshold, so a candidate EQUAL to the list's last entry never displaces it.)
// Equal rows of y give bit-equal D2 against any x_i (one norm kernel, one dot order), so exact duplicates come out by index.
// index_base is added to every stored index; column j is left out for row i when index_base + j == self_base + i (self_base >= 0).
// Unused tail entries stay (+inf, -1).
//
// Selection is by the Gram D2, which is accurate to an absolute 8 F u (|x|^2 + |y|^2): the k-th and the (k + 1)-th candidate can be
// exchanged only where they lie within twice that ceiling of each other.  What is REPORTED is refined by topk_refine_kernel: every
// kept pair recomputed as sum_f (x_if - y_jf)^2, the differences formed in fp64 from the fp32 values (exact), one wave per pair in
// norms_kernel's order, so an exact copy reports exactly 0.0 and not the 1e-13 the cancellation leaves; then the row's k entries are
// sorted again by (refined d2, index).
struct TopkConsumer {
    static constexpr int kIdxInts = kBM * kMaxK;
    const float *x, *y;
    const double *norm_x, *norm_y;
    double* out_d2;
    int* out_idx;
    int nx, ny, F, k, index_base;
    long long self_base;
    bool vec;
    double nr[4];
    int grow[4], self_col[4];

    __device__ int n_cols() const { return ny; }
    __device__ const float* row_a(int r) const { return r < nx ? x + (size_t)r * F : nullptr; }
    __device__ const float* row_b(int j) const { return j < ny ? y + (size_t)j * F : nullptr; }
    __device__ void init(double* scratch) {
        int* ilist = reinterpret_cast<int*>(scratch + kBM * kMaxK);
        for (int i = threadIdx.x; i < kBM * kMaxK; i += 256) {
            scratch[i] = __builtin_inf();
            ilist[i] = -1;
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            grow[r] = blockIdx.x * kBM + wave * 16 + (lane >> 4) + 4 * r;
            nr[r] = grow[r] < nx ? norm_x[grow[r]] : 0.0;
            const long long sc = self_base + grow[r] - index_base;       // the column that is row grow[r] itself
            self_col[r] = self_base >= 0 && sc >= 0 && sc < ny ? (int)sc : -1;
        }
        __syncthreads();
    }
    __device__ void tile(f64x4 (&acc)[kNT], int col0, double* scratch) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c16 = lane & 15, g = lane >> 4;
        volatile double* list = scratch + (wave * 16 + g) * kMaxK;      // + 4 reg * kMaxK: the lists of row g + 4 reg
        volatile int* ilist = reinterpret_cast<int*>(scratch + kBM * kMaxK) + (wave * 16 + g) * kMaxK;
        double thr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) thr[r] = list[4 * r * kMaxK + k - 1];
        bool pass = false;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int col = col0 + t * 16 + c16;
            const double nyj = col < ny ? norm_y[col] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = col < ny && grow[r] < nx && col != self_col[r];
                const double d = valid ? dist2(nr[r], nyj, acc[t][r]) : __builtin_inf();
                acc[t][r] = d;
                pass |= d < thr[r];
            }
        }
        if (!__any(pass)) return;
        // KnnConsumer's turns: one lane of a row at a time, a turn ends with a wavefront-scope fence and a wave barrier
#pragma unroll 1
        for (int s = 0; s < 16; ++s) {
            if (__ballot(c16 == s && pass) == 0) continue;       // wave-uniform: nobody holds a candidate in this turn
            if (c16 == s && pass) {
#pragma unroll
                for (int t = 0; t < kNT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double v = acc[t][r];
                        const int vi = index_base + col0 + t * 16 + c16;
                        volatile double* L = list + 4 * r * kMaxK;
                        volatile int* I = ilist + 4 * r * kMaxK;
                        const double last = L[k - 1];
                        if (v < last || (v == last && vi < I[k - 1])) {      // (+inf never enters: the tail's -1 is below any index)
                            int i = k - 1;
                            while (i > 0) {
                                const double u = L[i - 1];
                                const int ui = I[i - 1];
                                if (!(u > v || (u == v && ui > vi))) break;
                                L[i] = u;
                                I[i] = ui;
                                --i;
                            }
                            L[i] = v;
                            I[i] = vi;
                        }
                    }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __device__ void finish(double* scratch) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if ((lane & 15) != 0) return;
        volatile double* list = scratch + (wave * 16 + (lane >> 4)) * kMaxK;
        volatile int* ilist = reinterpret_cast<int*>(scratch + kBM * kMaxK) + (wave * 16 + (lane >> 4)) * kMaxK;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (grow[r] < nx)
                for (int i = 0; i < k; ++i) {
                    out_d2[(size_t)grow[r] * k + i] = list[4 * r * kMaxK + i];
                    out_idx[(size_t)grow[r] * k + i] = ilist[4 * r * kMaxK + i];
                }
    }
};

// The reported distances of TopkConsumer's pairs: a workgroup of k waves owns row i, wave w the pair (i, idx[i, w] - index_base):
// lane l sums (x_if - y_jf)^2 over f = l, l + 64, ... in order, then wave_sum_f64's tree (norms_kernel's order); an empty slot
// (idx -1) keeps +inf.  Thread 0 then sorts the row's k entries by (d2, index) and writes them back.
__global__ __launch_bounds__(64 * kMaxK) void topk_refine_kernel(const float* __restrict__ x, const float* __restrict__ y, int F, int k,
                                                                 int index_base, double* __restrict__ d2, int* __restrict__ idx) {
    __shared__ double sd[kMaxK];
    __shared__ int si[kMaxK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t row = blockIdx.x;
    const int gi = idx[row * k + w];
    double s = __builtin_inf();
    if (gi >= 0) {
        const float* px = x + row * F;
        const float* py = y + (size_t)(gi - index_base) * F;
        s = 0.0;
        for (int f = lane; f < F; f += 64) {
            const double v = (double)px[f] - (double)py[f];
            s = __fma_rn(v, v, s);
        }
        s = wave_sum_f64(s);
    }
    if (lane == 0) {
        sd[w] = s;
        si[w] = gi;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int a = 1; a < k; ++a) {
        const double v = sd[a];
        const int vi = si[a];
        int i = a;
        while (i > 0 && (sd[i - 1] > v || (sd[i - 1] == v && si[i - 1] > vi))) {
            sd[i] = sd[i - 1];
            si[i] = si[i - 1];
            --i;
        }
        sd[i] = v;
        si[i] = vi;
    }
    for (int a = 0; a < k; ++a) {
        d2[row * k + a] = sd[a];
        idx[row * k + a] = si[a];
    }
}

__global__ void poly_finish_kernel(const double* __restrict__ partial, int n_sums, int blocks, double* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sums) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)i * blocks + b];
    sums[i] = s;
}

bool can_vec(const float* p, int F) { return F % 4 == 0 && ((uintptr_t)p & 15) == 0; }

int launch_norms(const float* x, int n, int F, double* out, hipStream_t st) {
    hipLaunchKernelGGL(norms_kernel, dim3((unsigned)us_cdiv(n, 4)), dim3(256), 0, st, x, n, F, out);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

bool size_ok(int n) { return n >= 1 && n <= kMaxN; }

}  // namespace

extern "C" size_t uspace_metric_workspace_bytes(int nx, int ny, int n_subsets, int m) {
    if (!size_ok(nx) || ny < 0 || ny > kMaxN || n_subsets < 0 || n_subsets > 65535 || m < 0 || m > kMaxN) return 0;
    if (n_subsets > 0 && m < 1) return 0;
    return ((size_t)nx + (size_t)ny + (size_t)n_subsets * 3 * (size_t)us_cdiv(m, kBM)) * sizeof(double);
}

extern "C" int uspace_metric_knn_radius2(const float* x, int n, int F, int k, double* radius2, void* workspace,
                                         size_t workspace_bytes, uspace_stream_t stream) {
    if (!x || !radius2 || !workspace || !size_ok(n) || F < 1 || k < 1 || k > kMaxK || k > n - 1) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_metric_workspace_bytes(n, 0, 0, 0)) return USPACE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* norm = (double*)workspace;
    US_TRY(launch_norms(x, n, F, norm, st));
    KnnConsumer c = {};
    c.x = x;
    c.norm = norm;
    c.radius2 = radius2;
    c.n = n;
    c.F = F;
    c.k = k;
    c.vec = can_vec(x, F);
    hipLaunchKernelGGL(gram_kernel<KnnConsumer>, dim3((unsigned)us_cdiv(n, kBM)), dim3(256), 0, st, c);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_metric_manifold(const float* x, int nx, const float* y, int ny, int F, const double* radius2_y, int* count,
                                      double* min_d2, void* workspace, size_t workspace_bytes, uspace_stream_t stream) {
    if (!x || !y || !workspace || !size_ok(nx) || !size_ok(ny) || F < 1) return USPACE_ERR_ARG;
    if ((!count && !min_d2) || (count && !radius2_y)) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_metric_workspace_bytes(nx, ny, 0, 0)) return USPACE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* norm_x = (double*)workspace;
    double* norm_y = norm_x + nx;
    US_TRY(launch_norms(x, nx, F, norm_x, st));
    US_TRY(launch_norms(y, ny, F, norm_y, st));
    ManifoldConsumer c = {};
    c.x = x;
    c.y = y;
    c.norm_x = norm_x;
    c.norm_y = norm_y;
    c.radius2_y = count ? radius2_y : nullptr;
    c.count = count;
    c.min_d2 = min_d2;
    c.nx = nx;
    c.ny = ny;
    c.F = F;
    c.vec = can_vec(x, F) && can_vec(y, F);
    hipLaunchKernelGGL(gram_kernel<ManifoldConsumer>, dim3((unsigned)us_cdiv(nx, kBM)), dim3(256), 0, st, c);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_metric_poly_sums(const float* x, int nx, const float* y, int ny, int F, const int* idx_x, const int* idx_y,
                                       int n_subsets, int m, int degree, double gamma, double coef0, double* sums, void* workspace,
                                       size_t workspace_bytes, uspace_stream_t stream) {
    if (!x || !y || !idx_x || !idx_y || !sums || !workspace || !size_ok(nx) || !size_ok(ny) || F < 1) return USPACE_ERR_ARG;
    if (n_subsets < 1 || n_subsets > 65535 || m < 1 || m > nx || m > ny || degree < 1 || degree > 8) return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_metric_workspace_bytes(nx, ny, n_subsets, m)) return USPACE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = us_cdiv(m, kBM);
    PolyConsumer c = {};
    c.x = x;
    c.y = y;
    c.idx_x = idx_x;
    c.idx_y = idx_y;
    c.partial = (double*)workspace + nx + ny;
    c.m = m;
    c.F = F;
    c.degree = degree;
    c.gamma = gamma;
    c.coef0 = coef0;
    c.vec = can_vec(x, F) && can_vec(y, F);
    hipLaunchKernelGGL(gram_kernel<PolyConsumer>, dim3((unsigned)blocks, (unsigned)n_subsets, 3), dim3(256), 0, st, c);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(poly_finish_kernel, dim3((unsigned)us_cdiv(n_subsets * 3, 256)), dim3(256), 0, st, (const double*)c.partial,
                       n_subsets * 3, blocks, sums);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_metric_rbf_sums(const float* x, int nx, const float* y, int ny, int F, double gamma, int normalize,
                                      double* sums, void* workspace, size_t workspace_bytes, uspace_stream_t stream) {
    if (!x || !y || !sums || !workspace || !size_ok(nx) || !size_ok(ny) || F < 1) return USPACE_ERR_ARG;
    if (!(gamma >= 0.0) || gamma > DBL_MAX || (normalize != 0 && normalize != 1)) return USPACE_ERR_ARG;
    const int n_max = nx > ny ? nx : ny;
    if (workspace_bytes < uspace_metric_workspace_bytes(nx, ny, 1, n_max)) return USPACE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = us_cdiv(n_max, kBM);
    double* norm_x = (double*)workspace;
    double* norm_y = norm_x + nx;
    US_TRY(launch_norms(x, nx, F, norm_x, st));
    US_TRY(launch_norms(y, ny, F, norm_y, st));
    RbfConsumer c = {};
    c.x = x;
    c.y = y;
    c.norm_x = norm_x;
    c.norm_y = norm_y;
    c.partial = norm_y + ny;
    c.nx = nx;
    c.ny = ny;
    c.F = F;
    c.gamma = gamma;
    c.normalize = normalize != 0;
    c.vec = can_vec(x, F) && can_vec(y, F);
    hipLaunchKernelGGL(gram_kernel<RbfConsumer>, dim3((unsigned)blocks, 1, 3), dim3(256), 0, st, c);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(poly_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)c.partial, 3, blocks, sums);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}

extern "C" int uspace_metric_topk(const float* x, int nx, const float* y, int ny, int F, int k, int index_base, int self_base,
                                  double* d2, int* idx, void* workspace, size_t workspace_bytes, uspace_stream_t stream) {
    if (!x || !y || !d2 || !idx || !workspace || !size_ok(nx) || !size_ok(ny) || F < 1 || k < 1 || k > kMaxK) return USPACE_ERR_ARG;
    if (index_base < 0 || (long long)index_base + ny - 1 > INT_MAX || self_base < -1 || (long long)self_base + nx - 1 > INT_MAX)
        return USPACE_ERR_ARG;
    if (workspace_bytes < uspace_metric_workspace_bytes(nx, ny, 0, 0)) return USPACE_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* norm_x = (double*)workspace;
    double* norm_y = norm_x + nx;
    US_TRY(launch_norms(x, nx, F, norm_x, st));
    US_TRY(launch_norms(y, ny, F, norm_y, st));
    TopkConsumer c = {};
    c.x = x;
    c.y = y;
    c.norm_x = norm_x;
    c.norm_y = norm_y;
    c.out_d2 = d2;
    c.out_idx = idx;
    c.nx = nx;
    c.ny = ny;
    c.F = F;
    c.k = k;
    c.index_base = index_base;
    c.self_base = self_base;
    c.vec = can_vec(x, F) && can_vec(y, F);
    hipLaunchKernelGGL(gram_kernel<TopkConsumer>, dim3((unsigned)us_cdiv(nx, kBM)), dim3(256), 0, st, c);
    US_CHECK_LAUNCH();
    hipLaunchKernelGGL(topk_refine_kernel, dim3((unsigned)nx), dim3(64 * k), 0, st, x, y, F, k, index_base, d2, idx);
    US_CHECK_LAUNCH();
    return USPACE_OK;
}
