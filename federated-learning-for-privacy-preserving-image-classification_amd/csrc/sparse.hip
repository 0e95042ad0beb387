// sparse.hip — sparse top-k updates: packed (index, value) payloads and FedAvg from them.
// Closes the open end of DESIGN.md D20 (D21); the definition lives in include/fedhip.h.
//
// Reference: TopKSparsificationCompressor ships {'values', 'indices'} per layer
// (src/shared/compression.py:262-297) and rebuilds the dense tensor with _desparsify_tensor
// (:346-365).  Here a client's payload is two packed rows, idx (int32, segment-local flat index)
// and val (fp32): segment s sits at [koff[s], koff[s+1]), koff = exclusive prefix sum of seg_k,
// indices strictly ascending.
//
//   fh_topk_pack_rows      ordered stream compaction of the keep mask fh_topk_rows wrote: a count
//                          pass per (chunk, client), then a write pass that adds the counts of the
//                          segment's earlier chunks (integers: any order, the same sum) and places
//                          every kept element by wave ballot / prefix popcount.  No atomics.
//   fh_sparse_validate     per (segment, client): indices in range and strictly ascending.
//   fh_sparse_unpack_rows  out = base + d, d = val at the named indices and +0.0 elsewhere.
//   fh_sparse_fedavg       out = [out +] sum_k fl32(w_k) * fl32(base + d_k) without the dense rows.
//
// Work decomposition of the two consumers: every CHUNK-element chunk of the segment plan is cut
// into SP_SUBS pieces of SP_SUB elements, one workgroup each.  A piece's entries are one
// contiguous slice of the segment's sorted index list; its two ends come from binary searches.
// d lives in an LDS tile that is all +0.0 between clients.
//
// fh_sparse_fedavg keeps a piece's SP_SUB accumulators in registers (8 per lane) and walks the
// clients in row_index order.  Per batch of 64 clients two waves find all slice ends at once (one
// client per lane).  Then one barrier per client: the pass for client k scatters the entries of
// client k + 1 (already in registers) into the other tile, issues the loads of client k + 2,
// and accumulates client k from its tile, each lane re-zeroing the positions it has just read.
// HBM traffic: 8 bytes per payload entry, 8 per parameter.  The TU is built with
// -ffp-contract=off and has no fmaf: every fp32 operation is rounded on its own.
#include "fh_common.h"

namespace fh {

static constexpr int SP_CHUNK = 8192;  // == fh_compress_chunk_elems() (checked at launch)
static constexpr int SP_THREADS = 256;
static constexpr int SP_SUB = 2048;    // elements per workgroup of the consumers
static constexpr int SP_SUBS = SP_CHUNK / SP_SUB;
static constexpr int SP_VEC = SP_SUB / (SP_THREADS * 4);  // 4-element groups per lane
static constexpr int SP_PF = 2;        // payload entries per lane held in registers
static constexpr int SP_BATCH = 64;    // clients per slice search: one per lane

__device__ __forceinline__ int sp_seg_of_chunk(const int32_t* __restrict__ chunk_offsets, int nseg,
                                               int chunk) {
    int lo = 0, hi = nseg - 1;  // largest s with chunk_offsets[s] <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_offsets[mid] <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The chunk's element range [e0, e1) inside segment s of a row; s0 = the segment's first element.
struct SpRange {
    int s;
    int64_t s0, e0, e1;
};

__device__ __forceinline__ SpRange sp_range(const int64_t* __restrict__ seg_offsets,
                                            const int32_t* __restrict__ chunk_offsets, int nseg,
                                            int chunk) {
    SpRange r;
    r.s = sp_seg_of_chunk(chunk_offsets, nseg, chunk);
    r.s0 = seg_offsets[r.s];
    r.e0 = r.s0 + (int64_t)(chunk - chunk_offsets[r.s]) * SP_CHUNK;
    r.e1 = min(r.e0 + (int64_t)SP_CHUNK, seg_offsets[r.s + 1]);
    return r;
}

// One SP_SUB piece of a chunk: row elements [e0, e0 + len), segment-local indices [c0, c0 + len).
struct SpSub {
    int s, len, c0;
    int64_t e0;
};

__device__ __forceinline__ SpSub sp_sub(const int64_t* __restrict__ seg_offsets,
                                        const int32_t* __restrict__ chunk_offsets, int nseg,
                                        int block) {
    const SpRange r = sp_range(seg_offsets, chunk_offsets, nseg, block / SP_SUBS);
    SpSub g;
    g.s = r.s;
    g.e0 = r.e0 + (int64_t)(block % SP_SUBS) * SP_SUB;
    const int64_t e1 = min(g.e0 + (int64_t)SP_SUB, r.e1);
    g.len = e1 > g.e0 ? (int)(e1 - g.e0) : 0;
    g.c0 = (int)(g.e0 - r.s0);
    return g;
}

// First position p of [a, b) with idx[p] >= t (b when there is none); idx ascending there.
__device__ __forceinline__ int sp_lower_bound(const int32_t* __restrict__ idx, int a, int b,
                                              int t) {
    while (a < b) {
        const int m = (int)(((unsigned)a + (unsigned)b) >> 1);
        if (idx[m] < t) a = m + 1; else b = m;
    }
    return a;
}

// ------------------------------------------------------------------ pack
__global__ void __launch_bounds__(SP_THREADS)
sparse_count_kernel(const uint8_t* __restrict__ keep, int64_t k_cs,
                    const int64_t* __restrict__ seg_offsets,
                    const int32_t* __restrict__ chunk_offsets, int nseg, int nchunks,
                    int32_t* __restrict__ counts) {
    const int chunk = blockIdx.x, z = blockIdx.y;
    const SpRange rg = sp_range(seg_offsets, chunk_offsets, nseg, chunk);
    const uint8_t* kr = keep + z * k_cs;
    int c = 0;
    for (int64_t i = rg.e0 + threadIdx.x; i < rg.e1; i += SP_THREADS) c += kr[i] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int wc[SP_THREADS / 64];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[(int64_t)z * nchunks + chunk] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ void __launch_bounds__(SP_THREADS)
sparse_pack_kernel(const float* __restrict__ x, int64_t x_cs, const float* __restrict__ base,
                   int64_t b_cs, const uint8_t* __restrict__ keep, int64_t k_cs,
                   int32_t* __restrict__ idx, int64_t i_cs, float* __restrict__ val, int64_t v_cs,
                   int32_t* __restrict__ count_out, const int64_t* __restrict__ seg_offsets,
                   const int32_t* __restrict__ chunk_offsets, const int32_t* __restrict__ koff,
                   int nseg, int nchunks, const int32_t* __restrict__ counts) {
    const int chunk = blockIdx.x, z = blockIdx.y;
    const SpRange rg = sp_range(seg_offsets, chunk_offsets, nseg, chunk);
    const int s = rg.s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int s_before;
    __shared__ int wcnt[2][SP_THREADS / 64];
    if (wid == 0) {  // kept elements in the segment's earlier chunks
        int c = 0;
        for (int q = chunk_offsets[s] + lane; q < chunk; q += 64)
            c += counts[(int64_t)z * nchunks + q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_before = c;
    }
    __syncthreads();
    const int before = s_before;
    const int limit = koff[s + 1];  // nothing is written past the segment's slots
    const int pos0 = koff[s] + before;
    const float* xr = x + z * x_cs;
    const float* br = base ? base + z * b_cs : nullptr;
    const uint8_t* kr = keep + z * k_cs;
    int32_t* ir = idx + z * i_cs;
    float* vr = val + z * v_cs;
    int running = 0, it = 0;
    for (int64_t t0 = rg.e0; t0 < rg.e1; t0 += SP_THREADS, it ^= 1) {
        const int64_t i = t0 + threadIdx.x;
        const bool k = i < rg.e1 && kr[i] != 0;
        const uint64_t m = __ballot(k);
        const int lower = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[it][wid] = __popcll(m);
        __syncthreads();  // wcnt[it] is rewritten two iterations on, behind the next barrier
        int off = running;
        for (int w = 0; w < wid; ++w) off += wcnt[it][w];
        if (k) {
            const int p = pos0 + off + lower;
            if (p < limit) {
                ir[p] = (int32_t)(i - rg.s0);
                vr[p] = br ? xr[i] - br[i] : xr[i];
            }
        }
        running += wcnt[it][0] + wcnt[it][1] + wcnt[it][2] + wcnt[it][3];
    }
    if (count_out && threadIdx.x == 0 && chunk == chunk_offsets[s + 1] - 1)
        count_out[(int64_t)z * nseg + s] = before + running;  // one writer per (client, segment)
}

// ------------------------------------------------------------------ validate
__global__ void __launch_bounds__(SP_THREADS)
sparse_validate_kernel(const int32_t* __restrict__ idx, int64_t i_cs,
                       const int64_t* __restrict__ seg_lens, const int32_t* __restrict__ koff,
                       int nseg, int32_t* __restrict__ bad_out) {
    const int s = blockIdx.x, z = blockIdx.y;
    const int32_t* ir = idx + z * i_cs;
    const int a = koff[s], b = koff[s + 1];
    const int64_t len = seg_lens[s];
    int bad = 0;
    for (int p = a + (int)threadIdx.x; p < b; p += SP_THREADS) {
        const int32_t v = ir[p];
        if (v < 0 || (int64_t)v >= len) bad = 1;
        if (p > a && ir[p - 1] >= v) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) bad_out[(int64_t)z * nseg + s] = bad ? 1 : 0;
}

// ------------------------------------------------------------------ unpack
// out and base carry no __restrict__: out may be the base rows (every element is read before it
// is written, by the thread that writes it).
__global__ void __launch_bounds__(SP_THREADS)
sparse_unpack_kernel(const int32_t* __restrict__ idx, int64_t i_cs, const float* __restrict__ val,
                     int64_t v_cs, const float* base, int64_t b_cs, float* out, int64_t o_cs,
                     const int64_t* __restrict__ seg_offsets,
                     const int32_t* __restrict__ chunk_offsets, const int32_t* __restrict__ koff,
                     int nseg) {
    const int z = blockIdx.y;
    const SpSub g = sp_sub(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    if (g.len == 0) return;  // the whole workgroup: the chunk ends before this piece
    __shared__ float tile[SP_SUB];
    __shared__ int s_b[2];
    const int32_t* ir = idx + z * i_cs;
    const float* vr = val + z * v_cs;
    for (int q = threadIdx.x; q < SP_SUB; q += SP_THREADS) tile[q] = 0.f;
    if (threadIdx.x < 2)
        s_b[threadIdx.x] = sp_lower_bound(ir, koff[g.s], koff[g.s + 1],
                                          threadIdx.x == 0 ? g.c0 : g.c0 + g.len);
    __syncthreads();
    const int lo = s_b[0], hi = s_b[1];
    for (int p = lo + (int)threadIdx.x; p < hi; p += SP_THREADS) {
        const int li = ir[p] - g.c0;
        if ((unsigned)li < (unsigned)g.len) tile[li] = vr[p];
    }
    __syncthreads();
    const float* br = base ? base + z * b_cs : nullptr;
    float* orow = out + z * o_cs;
    for (int e = threadIdx.x; e < g.len; e += SP_THREADS) {
        const float d = tile[e];
        const int64_t i = g.e0 + e;
        orow[i] = br ? br[i] + d : d;
    }
}

// ------------------------------------------------------------------ sparse FedAvg
// The first SP_PF entries per lane of one client's slice, as tile positions (-1: none).
struct SpEntries {
    int li[SP_PF];
    float v[SP_PF];
};

__device__ __forceinline__ SpEntries sp_load(const int32_t* __restrict__ ir,
                                             const float* __restrict__ vr, int lo, int hi,
                                             int c0) {
    SpEntries r;
#pragma unroll
    for (int n = 0; n < SP_PF; ++n) {
        const int p = lo + (int)threadIdx.x + n * SP_THREADS;
        const bool in = p < hi;
        r.li[n] = in ? ir[p] - c0 : -1;
        r.v[n] = in ? vr[p] : 0.f;
    }
    return r;
}

__device__ __forceinline__ void sp_scatter(float* __restrict__ tile, const SpEntries& r,
                                           const int32_t* __restrict__ ir,
                                           const float* __restrict__ vr, int lo, int hi, int c0,
                                           int len) {
#pragma unroll
    for (int n = 0; n < SP_PF; ++n)
        if ((unsigned)r.li[n] < (unsigned)len) tile[r.li[n]] = r.v[n];
    for (int p = lo + (int)threadIdx.x + SP_PF * SP_THREADS; p < hi; p += SP_THREADS) {
        const int li = ir[p] - c0;  // a dense slice: more than SP_PF entries per lane
        if ((unsigned)li < (unsigned)len) tile[li] = vr[p];
    }
}

__global__ void __launch_bounds__(SP_THREADS)
sparse_fedavg_kernel(const int32_t* __restrict__ idx, int64_t i_cs, const float* __restrict__ val,
                     int64_t v_cs, const int32_t* __restrict__ row_index,
                     const float* __restrict__ weights, int C, const float* __restrict__ base,
                     const int64_t* __restrict__ seg_offsets,
                     const int32_t* __restrict__ chunk_offsets, const int32_t* __restrict__ koff,
                     int nseg, float* __restrict__ out, int accumulate) {
    const SpSub g = sp_sub(seg_offsets, chunk_offsets, nseg, blockIdx.x);
    if (g.len == 0) return;  // the whole workgroup
    __shared__ __attribute__((aligned(16))) float tile[2][SP_SUB];
    __shared__ int s_lo[SP_BATCH], s_hi[SP_BATCH];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int q = tid; q < 2 * SP_SUB; q += SP_THREADS) (&tile[0][0])[q] = 0.f;
    // lane's elements: e = (j * SP_THREADS + tid) * 4 + u
    float acc[SP_VEC][4], b[SP_VEC][4];
#pragma unroll
    for (int j = 0; j < SP_VEC; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = (j * SP_THREADS + tid) * 4 + u;
            const bool in = e < g.len;
            b[j][u] = in ? base[g.e0 + e] : 0.f;
            acc[j][u] = (in && accumulate) ? out[g.e0 + e] : 0.f;
        }
    const int ka = koff[g.s], kb = koff[g.s + 1];
    for (int k0 = 0; k0 < C; k0 += SP_BATCH) {
        const int nb = min(SP_BATCH, C - k0);
        __syncthreads();  // the tiles are zero and the last batch's slice ends are read
        if (wid < 2 && lane < nb) {  // wave 0: the slices' first entries, wave 1: their ends
            const int64_t r = row_index ? row_index[k0 + lane] : (k0 + lane);
            const int p = sp_lower_bound(idx + r * i_cs, ka, kb, wid == 0 ? g.c0 : g.c0 + g.len);
            if (wid == 0) s_lo[lane] = p; else s_hi[lane] = p;
        }
        __syncthreads();
        auto rows = [&](int k, const int32_t*& ir, const float*& vr) {
            const int64_t r = row_index ? row_index[k0 + k] : (k0 + k);
            ir = idx + r * i_cs;
            vr = val + r * v_cs;
        };
        const int32_t* ir;
        const float* vr;
        rows(0, ir, vr);
        SpEntries R = sp_load(ir, vr, s_lo[0], s_hi[0], g.c0);
        sp_scatter(tile[0], R, ir, vr, s_lo[0], s_hi[0], g.c0, g.len);
        if (nb > 1) {
            rows(1, ir, vr);
            R = sp_load(ir, vr, s_lo[1], s_hi[1], g.c0);
        }
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            // R holds client k + 1; its tile was re-zeroed in pass k - 1, before that barrier
            if (k + 1 < nb) {
                rows(k + 1, ir, vr);
                sp_scatter(tile[(k + 1) & 1], R, ir, vr, s_lo[k + 1], s_hi[k + 1], g.c0, g.len);
            }
            if (k + 2 < nb) {
                rows(k + 2, ir, vr);
                R = sp_load(ir, vr, s_lo[k + 2], s_hi[k + 2], g.c0);
            }
            const float w = weights[k0 + k];
            float* t = tile[k & 1];
#pragma unroll
            for (int j = 0; j < SP_VEC; ++j) {
                const int q = (j * SP_THREADS + tid) * 4;
                float d[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) d[u] = t[q + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) t[q + u] = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float xk = b[j][u] + d[u];  // the dense row's element
                    acc[j][u] = acc[j][u] + w * xk;   // rounded multiply, rounded add
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < SP_VEC; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = (j * SP_THREADS + tid) * 4 + u;
            if (e < g.len) out[g.e0 + e] = acc[j][u];
        }
}

static int sp_check_plan(const char* who, int32_t nclients, const int64_t* seg_offsets,
                         const int32_t* chunk_offsets, const int32_t* koff, int32_t nseg,
                         int32_t nchunks) {
    FH_REQUIRE(nclients >= 0 && nseg > 0 && nchunks >= nseg, "%s: bad shape", who);
    FH_REQUIRE(nclients == 0 || (seg_offsets && chunk_offsets && koff), "%s: null pointer", who);
    FH_REQUIRE(fh_compress_chunk_elems() == SP_CHUNK, "%s: chunk size mismatch", who);
    FH_REQUIRE((int64_t)nchunks * SP_SUBS <= 0x7FFFFFFFll, "%s: too many chunks", who);
    return FH_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int64_t fh_topk_pack_workspace(int32_t nclients, int32_t nchunks) {
    return (int64_t)nclients * nchunks * (int64_t)sizeof(int32_t);
}

extern "C" int fh_topk_pack_rows(const float* x, int64_t x_cs, const float* base, int64_t base_cs,
                                 const uint8_t* keep, int64_t keep_cs, int32_t* idx,
                                 int64_t idx_cs, float* val, int64_t val_cs, int32_t* count_out,
                                 int32_t nclients, const int64_t* seg_offsets,
                                 const int32_t* chunk_offsets, const int32_t* koff, int32_t nseg,
                                 int32_t nchunks, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = sp_check_plan("topk_pack_rows", nclients, seg_offsets, chunk_offsets, koff, nseg,
                               nchunks))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(x && keep && idx && val, "topk_pack_rows: null pointer");
    FH_REQUIRE(ws && (int64_t)ws_bytes >= fh_topk_pack_workspace(nclients, nchunks),
               "topk_pack_rows: workspace too small");
    int32_t* counts = reinterpret_cast<int32_t*>(ws);
    hipStream_t st = as_stream(stream);
    dim3 grid(nchunks, nclients);
    FH_LAUNCH(sparse_count_kernel, grid, dim3(SP_THREADS), 0, st, keep, keep_cs, seg_offsets,
              chunk_offsets, nseg, nchunks, counts);
    FH_LAUNCH_CHECK("topk_pack_rows/count");
    FH_LAUNCH(sparse_pack_kernel, grid, dim3(SP_THREADS), 0, st, x, x_cs, base, base_cs, keep,
              keep_cs, idx, idx_cs, val, val_cs, count_out, seg_offsets, chunk_offsets, koff, nseg,
              nchunks, counts);
    FH_LAUNCH_CHECK("topk_pack_rows/write");
    return FH_OK;
}

extern "C" int fh_sparse_validate(const int32_t* idx, int64_t idx_cs, int32_t nclients,
                                  const int64_t* seg_lens, const int32_t* koff, int32_t nseg,
                                  int32_t* bad_out, void* stream) {
    FH_REQUIRE(nclients >= 0 && nseg > 0, "sparse_validate: bad shape");
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(idx && seg_lens && koff && bad_out, "sparse_validate: null pointer");
    FH_LAUNCH(sparse_validate_kernel, dim3(nseg, nclients), dim3(SP_THREADS), 0,
              as_stream(stream), idx, idx_cs, seg_lens, koff, nseg, bad_out);
    FH_LAUNCH_CHECK("sparse_validate");
    return FH_OK;
}

extern "C" int fh_sparse_unpack_rows(const int32_t* idx, int64_t idx_cs, const float* val,
                                     int64_t val_cs, const float* base, int64_t base_cs,
                                     float* out, int64_t out_cs, int32_t nclients,
                                     const int64_t* seg_offsets, const int32_t* chunk_offsets,
                                     const int32_t* koff, int32_t nseg, int32_t nchunks,
                                     void* stream) {
    if (int rc = sp_check_plan("sparse_unpack_rows", nclients, seg_offsets, chunk_offsets, koff,
                               nseg, nchunks))
        return rc;
    if (nclients == 0) return FH_OK;
    FH_REQUIRE(idx && val && out, "sparse_unpack_rows: null pointer");
    FH_REQUIRE(out != base || base_cs != 0,
               "sparse_unpack_rows: out may not alias a broadcast base row");
    FH_LAUNCH(sparse_unpack_kernel, dim3(nchunks * SP_SUBS, nclients), dim3(SP_THREADS), 0,
              as_stream(stream), idx, idx_cs, val, val_cs, base, base_cs, out, out_cs, seg_offsets,
              chunk_offsets, koff, nseg);
    FH_LAUNCH_CHECK("sparse_unpack_rows");
    return FH_OK;
}

extern "C" int fh_sparse_fedavg(const int32_t* idx, int64_t idx_cs, const float* val,
                                int64_t val_cs, const int32_t* row_index, const float* weights,
                                int32_t num_clients, const float* base,
                                const int64_t* seg_offsets, const int32_t* chunk_offsets,
                                const int32_t* koff, int32_t nseg, int32_t nchunks, float* out,
                                int32_t accumulate, void* stream) {
    if (int rc = sp_check_plan("sparse_fedavg", 1, seg_offsets, chunk_offsets, koff, nseg, nchunks))
        return rc;
    FH_REQUIRE(num_clients >= 0, "sparse_fedavg: bad client count %d", num_clients);
    FH_REQUIRE(base && out && (num_clients == 0 || (idx && val && weights)),
               "sparse_fedavg: null pointer");
    FH_REQUIRE(out != base, "sparse_fedavg: out may not alias base");
    FH_LAUNCH(sparse_fedavg_kernel, dim3(nchunks * SP_SUBS), dim3(SP_THREADS), 0,
              as_stream(stream), idx, idx_cs, val, val_cs, row_index, weights, num_clients, base,
              seg_offsets, chunk_offsets, koff, nseg, out, accumulate);
    FH_LAUNCH_CHECK("sparse_fedavg");
    return FH_OK;
}
