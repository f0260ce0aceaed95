// occupancy_kernels.hip — site occupancy, unique starts and the motif overlap (Jaccard) sums of the hit records
// (SURVEY.md §8f): get_union_ranges + total_active_position (src/inference/_h4_overlap_ratio.jl:39-71), the get_uniq_pos
// counts (:1-15) and the pair sums of get_overlap_ratio (:86-117), over the record arrays the scan leaves in HBM.
//
// Per (motif, read) row the covered positions are a bitmap of W = ceil(L / 32) words; the outputs are sums over reads, so the
// reads are walked in chunks (the workspace bound) whose results add up, as shards do.
//   1. record pass: the start bit of every record goes into a start bitmap S (atomicOr), and a per-row key (largest start << 2 |
//      how often it occurs, saturating at 2) is kept by a compare-and-swap; records that leave 1..L or the call's reads raise a flag.
//   2. row pass: the quirk of union_ranges (below) on S, the unique-start count, then S dilated by len - 1 across word boundaries
//      in place: the coverage bitmap C, whose popcount is total_active_position's term.
//   3. overlap pass: sum over words of popcount(C_i & C_j) for i <= j, a K x K x (reads x W) "GEMM" in v_and_b32 + v_bcnt_u32_b32.
//
// Quirk kept (union_ranges, :48-56): `for i in eachindex(@view ranges[2:end])` runs i = 1 .. n-1 and pushes ranges[i], not
// ranges[i + 1], so of n >= 2 windows sorted by start ONE copy of the window with the largest start is never merged in.  A read
// with one window keeps it, and a largest start that occurs twice (a forward and a reverse-complement hit at the same l) is
// still covered by its other copy.  The row pass therefore drops the largest start from S iff it occurs once and another start
// exists in the row.  (The same kind of quirk as the `+ZᵀS` one the model keeps.)
//
// Exactness: every sum is an exact integer.  The reference accumulates the pair sum in Float32 (`overlap_ij = 0f0`); rounding our
// integer once to Float32 equals it bit for bit whenever it is below 2^24, above that the reference's own sum depends on the Dict
// iteration order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "api_common.h"
#include "scan_kernels.h"

using namespace motifs;

namespace {

constexpr int OCC_TILE = 64;          // overlap tile: 64 x 64 motif pairs per block, four waves of one 16-row band each
constexpr int OCC_KT = 32;            // words of C per k-step staged in LDS (rows of a chunk are padded to a multiple)
constexpr int OCC_LDW = OCC_KT + 4;   // LDS row pitch in words: 16 consecutive rows read as b128 hit 16 different bank groups
constexpr int OCC_BAND = 16;          // pair bands: a wave skips the 16 x 16 blocks below the diagonal and past K
constexpr int OCC_TARGET_BLOCKS = 2048;

// records: start bit into S and the row key (largest start << 2 | its count, saturating at 2).  minfo[m] = (row, len), row < 0: ignored.
__global__ __launch_bounds__(256) void k_occ_records(const HitRec* hits, int64_t n, const int2* minfo, int K_in, int64_t n0, int64_t N, int L,
                                                     int64_t c0, int nc, int W, int64_t pitch, uint32_t* rowkey, uint32_t* bits, int32_t* bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const HitRec h = hits[i];
        const uint32_t m = h.m - 1u;
        if (m >= (uint32_t)K_in) {                       // (no motif of this call: nothing to read its row from)
            *bad = 1;
            continue;
        }
        const int2 mi = minfo[m];
        if (mi.x < 0) continue;
        const int64_t rd = (int64_t)h.n - 1 - n0;        // the read within the call, 0-based
        if (rd < 0 || rd >= N || h.l < 1u || (int64_t)h.l + mi.y - 1 > L) {
            *bad = 1;
            continue;
        }
        const int64_t rc = rd - c0;                      // ... within this chunk
        if (rc < 0 || rc >= nc) continue;
        uint32_t* key = rowkey + (size_t)mi.x * nc + rc;
        const uint32_t l = h.l;
        uint32_t old = __hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {
            const uint32_t ol = old >> 2;
            if (l < ol) break;
            uint32_t nw;
            if (l > ol) nw = (l << 2) | 1u;
            else if ((old & 3u) >= 2u) break;
            else nw = old + 1u;
            const uint32_t prev = atomicCAS(key, old, nw);
            if (prev == old) break;
            old = prev;
        }
        const uint32_t p = l - 1u;
        atomicOr(bits + (size_t)mi.x * pitch + (size_t)rc * W + (p >> 5), 1u << (p & 31u));
    }
}

// OR over s = 0 .. d of x << s, within one word
__device__ __forceinline__ uint32_t smear(uint32_t x, int d) {
    if (d >= 31) return x ? (~0u << __builtin_ctz(x)) : 0u;
    uint32_t r = x;
    int span = 1;                                        // r = OR over s < span of x << s
    while (2 * span <= d + 1) {
        r |= r << span;
        span *= 2;
    }
    if (span < d + 1) r |= r << (d + 1 - span);
    return r;
}

__device__ __forceinline__ unsigned long long block_sum_256(unsigned long long v, unsigned long long* red) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// rows: one thread per (motif row r, read); blocks of 256 reads of ONE row r, so a block adds one total per output
__global__ __launch_bounds__(256) void k_occ_rows(const uint32_t* rowkey, const int32_t* rowlen, int nc, int nbx, int W, int64_t pitch,
                                                  uint32_t* bits, unsigned long long* occupied, unsigned long long* uniq) {
    __shared__ unsigned long long red[8];
    const int r = blockIdx.x / nbx;
    const int rd = (blockIdx.x - r * nbx) * 256 + threadIdx.x;
    unsigned long long occ = 0, uq = 0;
    const uint32_t key = rd < nc ? rowkey[(size_t)r * nc + rd] : 0u;
    if (key) {
        const int mx = (int)(key >> 2) - 1;              // largest start, 0-based
        const bool once = (key & 3u) == 1u;
        const int d = rowlen[r] - 1;
        const int jm = mx >> 5;
        const uint32_t mbit = 1u << (mx & 31);
        uint32_t* row = bits + (size_t)r * pitch + (size_t)rd * W;
        bool other = false;
        long long last = -(1ll << 40);                   // largest start of the words before this one
        for (int j = 0; j < W; j++) {
            uint32_t s = row[j];
            uq += __builtin_popcount(s);                 // distinct starts (get_uniq_pos)
            if (j < jm) {
                other |= s != 0u;
            } else if (j == jm) {
                other |= (s & ~mbit) != 0u;
                if (once && other) s &= ~mbit;           // union_ranges never merges in the last window (see the top of this file)
            }
            uint32_t c = smear(s, d);
            const long long nb = last + d - 32ll * j + 1;  // positions of this word the earlier windows reach
            if (nb > 0) c |= nb >= 32 ? ~0u : ((1u << nb) - 1u);
            if (s) last = 32ll * j + 31 - __builtin_clz(s);
            row[j] = c;
            occ += __builtin_popcount(c);
        }
    }
    const unsigned long long so = block_sum_256(occ, red);
    const unsigned long long su = block_sum_256(uq, red + 4);
    if (threadIdx.x == 0) {
        if (so) atomicAdd(occupied + r, so);
        if (uniq && su) atomicAdd(uniq + r, su);
    }
}

// popcount(x) + acc in ONE v_bcnt_u32_b32 (left to itself the compiler counts into 0 and sums the counts with v_add3_u32: 10 vector
// instructions per 4 words and pair instead of 8)
__device__ __forceinline__ uint32_t bcnt_add(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// overlap: blockIdx = split * tiles + tile (the tiles of one k range run side by side and share its rows in the caches).  Tile
// (ti <= tj) covers rows ti*64.. x columns tj*64..; wave w takes the 16-row band w, a lane 4 rows x 4 columns 16 apart
// (columns c, c+16, c+32, c+48), so a 16 x 16 block below the diagonal or past K is skipped by the whole wave.  int32 partials
// (a block adds at most 2^21 k-steps x 1 024 bits), then one 64-bit atomic per pair and block into P (upper triangle).
__global__ __launch_bounds__(256) void k_occ_overlap(const uint32_t* bits, int64_t pitch, int K, int K16, int nt, int tiles, int splits,
                                                     int64_t ksteps, unsigned long long* P) {
    __shared__ __attribute__((aligned(16))) uint32_t sA[OCC_TILE * OCC_LDW];
    __shared__ __attribute__((aligned(16))) uint32_t sB[OCC_TILE * OCC_LDW];
    const int t = blockIdx.x % tiles, sp = blockIdx.x / tiles;
    int ti = 0, tt = t;
    while (tt >= nt - ti) tt -= nt - ti, ti++;
    const int tj = ti + tt;
    const int64_t kb = ksteps * sp / splits, ke = ksteps * (sp + 1) / splits;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r4 = lane >> 4, c = lane & 15;
    const int band_r = ti * 4 + w;
    int lm = 0;                                          // live column bands of this wave (a wave-uniform mask: scalar branches below)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int band_c = tj * 4 + j;
        lm |= (band_r * OCC_BAND < K && band_c * OCC_BAND < K && band_c >= band_r) << j;
    }
    lm = __builtin_amdgcn_readfirstlane(lm);
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; j++) live[j] = (lm >> j) & 1;
    const bool any = lm != 0;
    // staging: 64 rows x 8 uint4 per operand and k-step, two of each per thread
    int srow[2], scol[2];
    bool okA[2], okB[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int idx = tid + 256 * q;
        srow[q] = idx >> 3;
        scol[q] = (idx & 7) * 4;
        okA[q] = ti * OCC_TILE + srow[q] < K16;
        okB[q] = tj * OCC_TILE + srow[q] < K16;
    }
    const uint32_t* gA = bits + (size_t)ti * OCC_TILE * pitch;
    const uint32_t* gB = bits + (size_t)tj * OCC_TILE * pitch;
    uint4 ra[2], rb[2];
    auto fetch = [&](int64_t k) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const size_t off = (size_t)srow[q] * pitch + (size_t)k * OCC_KT + scol[q];
            ra[q] = okA[q] ? *(const uint4*)(gA + off) : make_uint4(0u, 0u, 0u, 0u);
            rb[q] = okB[q] ? *(const uint4*)(gB + off) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    uint32_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0u;
    if (kb < ke) fetch(kb);
    for (int64_t k = kb; k < ke; k++) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; q++) {
            *(uint4*)(sA + srow[q] * OCC_LDW + scol[q]) = ra[q];
            *(uint4*)(sB + srow[q] * OCC_LDW + scol[q]) = rb[q];
        }
        __syncthreads();
        if (k + 1 < ke) fetch(k + 1);                    // in flight under this step's popcounts
        if (!any) continue;
#pragma unroll
        for (int g = 0; g < OCC_KT / 4; g++) {
            uint4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = *(const uint4*)(sA + (w * OCC_BAND + r4 * 4 + i) * OCC_LDW + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = *(const uint4*)(sB + (j * OCC_BAND + c) * OCC_LDW + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (!live[j]) continue;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    uint32_t v = acc[i][j];
                    v = bcnt_add(a[i].x & b[j].x, v);
                    v = bcnt_add(a[i].y & b[j].y, v);
                    v = bcnt_add(a[i].z & b[j].z, v);
                    v = bcnt_add(a[i].w & b[j].w, v);
                    acc[i][j] = v;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!live[j]) continue;
        const int gj = (tj * 4 + j) * OCC_BAND + c;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int gi = band_r * OCC_BAND + r4 * 4 + i;
            if (gi < K && gj < K && gi <= gj && acc[i][j]) atomicAdd(P + (size_t)gi * K + gj, (unsigned long long)acc[i][j]);
        }
    }
}

// out[i][j] += P[min(i, j)][max(i, j)]
__global__ void k_occ_mirror(const unsigned long long* P, int K, int64_t* out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)K * K) return;
    const int i = (int)(e / K), j = (int)(e - (int64_t)i * K);
    out[e] += (int64_t)(i <= j ? P[(size_t)i * K + j] : P[(size_t)j * K + i]);
}

int invalid(const char* why) {
    set_error("motifs_hits_occupancy_dev: %s", why);
    return MOTIFS_ERR_INVALID;
}

}  // namespace

extern "C" int motifs_hits_occupancy_dev(motifs_ctx* c, const motifs_hit* hits_a_dev, int64_t n_a, const motifs_hit* hits_b_dev, int64_t n_b,
                                         int64_t n0, int64_t N, int L, const int64_t* lens, int K_in, const int32_t* motif_map, int K_out,
                                         int64_t* occupied_dev, int64_t* uniq_dev, int64_t* overlap_dev) {
    if (!c) return invalid("null context");
    if (n_a < 0 || n_b < 0 || (n_a > 0 && !hits_a_dev) || (n_b > 0 && !hits_b_dev)) return invalid("bad record arrays");
    if (n0 < 0 || N < 0 || L < 1 || L >= (1 << 30)) return invalid("bad n0 / N / L");
    if (K_in < 1 || K_out < 1 || !lens || !occupied_dev) return invalid("bad K_in / K_out / lens / occupied_dev");
    if (!motif_map && K_out != K_in) return invalid("motif_map NULL needs K_out == K_in");
    std::vector<int32_t> minfo(2 * (size_t)K_in), rowlen((size_t)K_out, 1);
    std::vector<char> taken((size_t)K_out, 0);
    for (int m = 0; m < K_in; m++) {
        const int32_t row = motif_map ? motif_map[m] : m;
        if (row < -1 || row >= K_out) return invalid("motif_map entry out of range");
        minfo[2 * m] = row;
        minfo[2 * m + 1] = (int32_t)std::min<int64_t>(std::max<int64_t>(lens[m], 0), (int64_t)L + 1);
        if (row < 0) continue;
        if (lens[m] < 1) return invalid("a used motif has a length below 1");
        if (taken[row]) return invalid("two motifs map to one row");
        taken[row] = 1;
        rowlen[row] = minfo[2 * m + 1];
    }
    if (N == 0) return n_a + n_b > 0 ? invalid("records but no reads") : MOTIFS_OK;
    MOTIFS_HIP_CHECK(hipSetDevice(c->device));

    const bool want_pairs = overlap_dev != nullptr;
    const int W = (L + 31) / 32;
    const int K16 = want_pairs ? (K_out + OCC_BAND - 1) / OCC_BAND * OCC_BAND : K_out;
    // a chunk of nc reads: 4 nc K_out bytes of row keys + 4 K16 pitch bytes of bitmap, pitch = nc W rounded up to OCC_KT words
    const int64_t per_read = 4 * ((int64_t)K_out + (int64_t)K16 * W);
    const int64_t Nc = std::max<int64_t>(1, std::min<int64_t>({N, (int64_t)(c->ws_limit / (size_t)per_read), (int64_t)1 << 30}));
    const int64_t pitch_max = (Nc * W + OCC_KT - 1) / OCC_KT * OCC_KT;
    MOTIFS_HIP_CHECK(c->occ_ws.reserve((size_t)4 * K_out * Nc + (size_t)4 * K16 * pitch_max + 256));
    MOTIFS_HIP_CHECK(c->occ_small.reserve(minfo.size() * 4 + rowlen.size() * 4 + 64));
    if (want_pairs) MOTIFS_HIP_CHECK(c->occ_pairs.reserve((size_t)8 * K_out * K_out));
    uint32_t* rowkey = (uint32_t*)c->occ_ws.p;
    uint32_t* bits = (uint32_t*)((char*)c->occ_ws.p + ((size_t)4 * K_out * Nc + 255) / 256 * 256);
    int2* d_minfo = (int2*)c->occ_small.p;
    int32_t* d_rowlen = (int32_t*)(d_minfo + K_in);
    int32_t* d_bad = d_rowlen + K_out;
    unsigned long long* P = (unsigned long long*)c->occ_pairs.p;
    MOTIFS_HIP_CHECK(hipMemcpyAsync(d_minfo, minfo.data(), minfo.size() * 4, hipMemcpyHostToDevice, c->stream));
    MOTIFS_HIP_CHECK(hipMemcpyAsync(d_rowlen, rowlen.data(), rowlen.size() * 4, hipMemcpyHostToDevice, c->stream));
    MOTIFS_HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, c->stream));
    if (want_pairs) MOTIFS_HIP_CHECK(hipMemsetAsync(P, 0, (size_t)8 * K_out * K_out, c->stream));

    for (int64_t c0 = 0; c0 < N; c0 += Nc) {
        const int nc = (int)std::min<int64_t>(Nc, N - c0);
        const int64_t pitch = ((int64_t)nc * W + OCC_KT - 1) / OCC_KT * OCC_KT;
        {
            KernelTimer tm(c, KS_OCC_RECORDS);
            MOTIFS_HIP_CHECK(hipMemsetAsync(rowkey, 0, (size_t)4 * K_out * nc, c->stream));
            MOTIFS_HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)4 * K16 * pitch, c->stream));
            const motifs_hit* hs[2] = {hits_a_dev, hits_b_dev};
            const int64_t ns[2] = {n_a, n_b};
            for (int s = 0; s < 2; s++)
                if (ns[s] > 0)
                    hipLaunchKernelGGL(k_occ_records, dim3((unsigned)std::min<int64_t>((ns[s] + 255) / 256, 8192)), dim3(256), 0, c->stream,
                                       (const HitRec*)hs[s], ns[s], (const int2*)d_minfo, K_in, n0, N, L, c0, nc, W, pitch, rowkey, bits, d_bad);
        }
        {
            KernelTimer tm(c, KS_OCC_ROWS);
            const int nbx = (nc + 255) / 256;
            hipLaunchKernelGGL(k_occ_rows, dim3((unsigned)((int64_t)K_out * nbx)), dim3(256), 0, c->stream, rowkey, d_rowlen, nc, nbx, W, pitch,
                               bits, (unsigned long long*)occupied_dev, (unsigned long long*)uniq_dev);
        }
        if (want_pairs) {
            KernelTimer tm(c, KS_OCC_OVERLAP);
            const int nt = (K_out + OCC_TILE - 1) / OCC_TILE;
            const int tiles = nt * (nt + 1) / 2;
            const int64_t ksteps = pitch / OCC_KT;
            int64_t splits = std::max<int64_t>((OCC_TARGET_BLOCKS + tiles - 1) / tiles, (ksteps + (1 << 21) - 1) >> 21);
            splits = std::max<int64_t>(1, std::min<int64_t>(splits, ksteps));
            hipLaunchKernelGGL(k_occ_overlap, dim3((unsigned)(tiles * splits)), dim3(256), 0, c->stream, bits, pitch, K_out, K16, nt, tiles,
                               (int)splits, ksteps, P);
        }
        MOTIFS_HIP_CHECK(hipGetLastError());
    }
    if (want_pairs) {
        KernelTimer tm(c, KS_OCC_OVERLAP);
        const int64_t e = (int64_t)K_out * K_out;
        hipLaunchKernelGGL(k_occ_mirror, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, c->stream, P, K_out, overlap_dev);
    }
    MOTIFS_HIP_CHECK(hipGetLastError());
    int32_t* h_bad = (int32_t*)c->pinned + 40;
    MOTIFS_HIP_CHECK(hipMemcpyAsync(h_bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    MOTIFS_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (*h_bad) return invalid("a record's window leaves 1..L, its read leaves n0+1..n0+N, or its m leaves 1..K_in");
    return MOTIFS_OK;
}
