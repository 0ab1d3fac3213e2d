// ukm_fastx.hip — ukm_fastx: FASTA/Q text to the bases and record offsets the encode kernels take, held byte for byte to
// host/seqtext.hpp's parse_fastx.  The call handles the longest prefix inside the device's grammar and says where it stopped
// (include/unikmer_hip.h); byte images and the size-then-write protocol are ukm_bytes.h's.  Tiles of FASTX_TILE text bytes,
// one byte in front (does the tile's first byte start a line?) and one behind (is a CR followed by an LF?); a lane looks at
// FX_VT consecutive bytes.  No lane's work depends on the length of a line or a record.
//
// FASTA.  Whether a byte is name or sequence depends on the first byte of its line, which may lie many tiles back.  A tile
// (and, inside a tile, a lane) either SETS the state of the line that runs out of it -- it holds a line start; the last one
// decides -- or PASSES the state it was given.  Composition is "the last setter wins":
//   fa_summary_kernel  per tile: set-header / set-sequence / pass, the number of header lines (SizeScan of the records), and by
//                      atomicMin / atomicMax the first header and the last header,
//   fa_state_kernel    one workgroup: a setter's rank among the setters is an exclusive sum (block_excl_scan_u32), the
//                      setters leave their state in LDS by rank, tile i takes the state of rank - 1 (or the carry),
//   fa_tile_kernel<0>  per tile, with its incoming state: the same composition across the lanes, then the kept bytes
//                      (SizeScan of the bases); a line in front of the first header that is not empty by atomicMin (garbage),
//   fa_tile_kernel<1>  again, compacting the kept bytes into an LDS image flushed at the tile's offset; a header line's lane
//                      stores the record's offset in the bases and the header's offset in the text.
// FASTQ.  A line's role is its index mod 4: the line-end table.
//   fq_count_kernel    LF per tile (SizeScan of the lines); is the last byte an LF?
//   fq_table_kernel    the position of every LF, in order; a blank inside a sequence line flags its group (atomicMin),
//   fq_group_kernel    one thread per group of four lines: the four rules from the table and five bytes of text; the length
//                      of the sequence line, the offset of the header; the first group that breaks a rule by atomicMin,
//   (ukm_dev_exclusive_scan_u64 over the lengths: the record offsets)
//   fq_result_kernel   one thread: the good groups, their bases, the byte behind them,
//   fq_write_kernel    per tile of the consumed prefix: line index from the LF counts, the bytes of the good groups'
//                      sequence lines compacted into the image; the tile's place follows from the table.
#include "ukm_bytes.h"

namespace {

constexpr int FASTX_TILE = 4096;  // text bytes per tile
constexpr int FX_VT = FASTX_TILE / NT;
constexpr int FX_IMG = FASTX_TILE + 32;  // + a byte in front, one behind, up to 15 of alignment shift, rounded to 16
static_assert(FX_VT == 16 && FX_IMG % 16 == 0 && FX_IMG >= FASTX_TILE + 2 + 15, "LDS images are whole 16-byte words");
static_assert(FASTX_TILE < 65536, "kept bytes and header lines of a tile share one scanned word");

enum : u32 { ST_SEQ = 0, ST_HDR = 1 };
enum : int { AUX_FIRST_HDR = 0, AUX_GARBAGE = 1, AUX_LAST_HDR1 = 2, AUX_BAD_GROUP = 0, AUX_WORDS = 4 };

// the tile's text in LDS; returns B with B[i] = text[start + i] for -1 (where start > 0) <= i <= FASTX_TILE (where the text goes on)
__device__ inline const u8 *fx_load(const u8 *text, u64 n_bytes, u64 start, uint4 *img, int tid) {
    const u64 lo = start ? start - 1 : 0;
    const u64 hi = n_bytes - start <= (u64)FASTX_TILE ? n_bytes : start + (u64)FASTX_TILE + 1;
    const int shift = load_image(text, lo, (u32)(hi - lo), img, tid);
    return (const u8 *)img + shift + (start - lo);
}

// a lane's bytes: c[j + 1] = text[at + j] for j < m, c[0] the byte in front (an LF in front of the text: offset 0 starts a
// line), c[m + 1] the byte behind (0 behind the text: no LF)
struct FxLane {
    u8 c[FX_VT + 2];
    int m;
    u64 at;
};
__device__ inline void fx_lane(const u8 *B, u64 n_bytes, u64 start, int tid, FxLane &L) {
    const int p0 = tid * FX_VT;
    L.at = start + (u64)p0;
    L.m = L.at >= n_bytes ? 0 : (n_bytes - L.at < (u64)FX_VT ? (int)(n_bytes - L.at) : FX_VT);
    L.c[0] = L.at == 0 ? (u8)'\n' : (L.m > 0 ? B[p0 - 1] : (u8)0);
#pragma unroll
    for (int j = 0; j < FX_VT; j++) L.c[j + 1] = j < L.m ? B[p0 + j] : (u8)0;
    L.c[FX_VT + 1] = L.at + (u64)FX_VT < n_bytes ? B[p0 + FX_VT] : (u8)0;
}
// a byte of a sequence line that is kept: not the LF, not a blank, not a CR in front of an LF
__device__ inline bool fx_base(u32 c, u32 next) { return c != '\n' && c != ' ' && c != '\t' && !(c == '\r' && next == '\n'); }

// does the lane hold a line start, and what kind of line runs out of it then
__device__ inline bool fa_setter(const FxLane &L, u32 *cls) {
    bool set = false;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j < L.m && L.c[j] == '\n') {
            set = true;
            *cls = L.c[j + 1] == '>' ? ST_HDR : ST_SEQ;
        }
    }
    return set;
}

__global__ __launch_bounds__(NT) void fa_summary_kernel(const u8 *text, u64 n_bytes, u32 *tsum, u32 *hsums, u64 *aux) {
    __shared__ uint4 s_img[FX_IMG / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    __shared__ u32 s_last;
    __shared__ unsigned long long s_first, s_lasth;
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * FASTX_TILE;
    if (tid == 0) {
        s_last = 0;
        s_first = ~0ull;
        s_lasth = 0;
    }
    const u8 *B = fx_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    FxLane L;
    fx_lane(B, n_bytes, start, tid, L);
    u32 h = 0, cls = ST_SEQ;
    bool set = false;
    u64 first = ~0ull, lasth = 0;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j >= L.m || L.c[j] != '\n') continue;
        const u32 c = L.c[j + 1];
        const u64 p = L.at + (u64)j;
        set = true;
        if (c == '>') {
            cls = ST_HDR;
            h++;
            if (first == ~0ull) first = p;
            lasth = p + 1;
        } else {
            cls = ST_SEQ;
        }
    }
    if (set) atomicMax(&s_last, (u32)tid * 2u + cls + 1u);
    if (first != ~0ull) atomicMin(&s_first, (unsigned long long)first);
    if (lasth) atomicMax(&s_lasth, (unsigned long long)lasth);
    u32 total;
    (void)block_excl_scan_u32<NT>(h, s_scan, &total);  // (its barriers also order the LDS atomics in front of the reads below)
    if (tid == 0) {
        hsums[blockIdx.x] = total;
        tsum[blockIdx.x] = s_last ? ((s_last - 1u) & 1u) + 1u : 0u;
        if (s_first != ~0ull) atomicMin((unsigned long long *)&aux[AUX_FIRST_HDR], s_first);
        if (s_lasth) atomicMax((unsigned long long *)&aux[AUX_LAST_HDR1], s_lasth);
    }
}

// one workgroup; tsum[i]: 0 pass, 1 + state set -> the state at tile i's first byte where that byte does not start a line
__global__ __launch_bounds__(NT) void fa_state_kernel(u32 *tsum, u64 ntiles) {
    __shared__ u32 s_scan[SCAN_LDS];
    __shared__ u8 s_cls[NT];
    const int tid = (int)threadIdx.x;
    u32 carry = ST_SEQ;
    for (u64 i0 = 0; i0 < ntiles; i0 += NT) {
        const u64 i = i0 + (u64)tid;
        const u32 v = i < ntiles ? tsum[i] : 0u;
        u32 total;
        const u32 r = block_excl_scan_u32<NT>(v ? 1u : 0u, s_scan, &total);
        if (v) s_cls[r] = (u8)(v - 1u);
        __syncthreads();
        if (i < ntiles) tsum[i] = r ? (u32)s_cls[r - 1] : carry;
        if (total) carry = s_cls[total - 1];
        __syncthreads();
    }
}

// the state at the lane's first byte: the last setter among the lanes in front, else the tile's
__device__ inline u32 fa_lane_state(const FxLane &L, u32 tile_in, u32 *s_scan, u8 *s_cls) {
    u32 cls = ST_SEQ;
    const bool set = fa_setter(L, &cls);
    u32 total;
    const u32 r = block_excl_scan_u32<NT>(set ? 1u : 0u, s_scan, &total);
    if (set) s_cls[r] = (u8)cls;
    __syncthreads();
    return r ? (u32)s_cls[r - 1] : tile_in;
}

// WRITE = false: the kept bytes of every tile into bsums.  WRITE = true: the bases to out_bases, and for header line j of the
// text rec_off[j] (j <= n_rec) and hdr_off[j] (j < n_rec); tail_rec: rec_off[n_rec] = n_bases belongs to no header line.
template <bool WRITE>
__global__ __launch_bounds__(NT) void fa_tile_kernel(const u8 *text, u64 n_bytes, int last, const u32 *tin, u64 *aux, u32 *bsums,
                                                     const u64 *boffs, const u64 *roffs, u8 *out_bases, u64 *rec_off, u64 *hdr_off,
                                                     u64 n_rec, u64 n_bases, int tail_rec) {
    __shared__ uint4 s_img[FX_IMG / 16];
    __shared__ uint4 s_out[WRITE ? FX_IMG / 16 : 1];
    __shared__ u32 s_scan[SCAN_LDS];
    __shared__ u8 s_cls[NT];
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * FASTX_TILE;
    // without LAST the text counts up to the start of its last header line
    const u64 lh1 = aux[AUX_LAST_HDR1];
    const u64 limit = last ? n_bytes : (lh1 ? lh1 - 1 : 0);
    const u64 first_hdr = aux[AUX_FIRST_HDR];  // (~0: none) lines in front of it must be empty
    const u8 *B = fx_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    FxLane L;
    fx_lane(B, n_bytes, start, tid, L);
    const u32 st = fa_lane_state(L, tin[blockIdx.x], s_scan, s_cls);
    u32 kept = 0, hdrs = 0, cur = st;
    u64 garb = ~0ull;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j >= L.m) continue;
        const u32 c = L.c[j + 1];
        if (L.c[j] == '\n') {
            cur = c == '>' ? ST_HDR : ST_SEQ;
            hdrs += cur;
            const u64 p = L.at + (u64)j;
            if (!WRITE && p < first_hdr && garb == ~0ull) {
                // in front of the first header only empty lines pass; a CR that ends a text with more behind it is undecided
                const u32 nx = L.c[j + 2];
                const bool empty = c == '\n' || (c == '\r' && (nx == '\n' || (p + 1 == n_bytes && !last)));
                if (!empty) garb = p;
            }
        }
        kept += (cur == ST_SEQ && L.at + (u64)j < limit && fx_base(c, L.c[j + 2])) ? 1u : 0u;
    }
    u32 total;
    const u32 excl = block_excl_scan_u32<NT>(kept | (hdrs << 16), s_scan, &total);
    if (!WRITE) {
        if (garb != ~0ull) atomicMin((unsigned long long *)&aux[AUX_GARBAGE], (unsigned long long)garb);
        if (tid == 0) bsums[blockIdx.x] = total & 0xFFFFu;
        return;
    }
    const u64 b0 = boffs[blockIdx.x];
    u8 *dst = out_bases + b0;
    int shift;
    u8 *O = image_at(dst, s_out, &shift);
    u32 k = excl & 0xFFFFu;
    u64 jrec = roffs[blockIdx.x] + (u64)(excl >> 16);
    cur = st;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j >= L.m) continue;
        const u32 c = L.c[j + 1];
        if (L.c[j] == '\n') {
            cur = c == '>' ? ST_HDR : ST_SEQ;
            if (cur == ST_HDR) {
                if (jrec <= n_rec) rec_off[jrec] = b0 + (u64)k;
                if (jrec < n_rec && hdr_off) hdr_off[jrec] = L.at + (u64)j;
                jrec++;
            }
        }
        if (cur == ST_SEQ && L.at + (u64)j < limit && fx_base(c, L.c[j + 2])) O[k++] = (u8)c;
    }
    if (tail_rec && blockIdx.x == 0 && tid == 0) rec_off[n_rec] = n_bases;
    __syncthreads();
    if (total & 0xFFFFu) flush_image(dst, total & 0xFFFFu, s_out, shift, tid);
}

// ---- FASTQ ------------------------------------------------------------------------------------------------------------------
__device__ inline u32 fq_lane_lf(const FxLane &L) {
    u32 n = 0;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) n += (j < L.m && L.c[j + 1] == '\n') ? 1u : 0u;
    return n;
}

// ctl[1] (zero before): 1 where the text does not end in an LF
__global__ __launch_bounds__(NT) void fq_count_kernel(const u8 *text, u64 n_bytes, u32 *sums, u64 *ctl) {
    __shared__ uint4 s_img[FX_IMG / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * FASTX_TILE;
    const u8 *B = fx_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    FxLane L;
    fx_lane(B, n_bytes, start, tid, L);
    if (L.m > 0 && L.at + (u64)L.m == n_bytes && B[tid * FX_VT + L.m - 1] != '\n') ctl[1] = 1;
    u32 total;
    (void)block_excl_scan_u32<NT>(fq_lane_lf(L), s_scan, &total);
    if (tid == 0) sums[blockIdx.x] = total;
}

// lf[i] = the position of LF i; virt: the end of the text stands for one more.  A blank inside line 4 g + 1 flags group g.
__global__ __launch_bounds__(NT) void fq_table_kernel(const u8 *text, u64 n_bytes, const u64 *loffs, u64 n_lf, int virt, u64 *lf, u64 *aux) {
    __shared__ uint4 s_img[FX_IMG / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * FASTX_TILE;
    const u8 *B = fx_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    FxLane L;
    fx_lane(B, n_bytes, start, tid, L);
    u32 total;
    u64 idx = loffs[blockIdx.x] + (u64)block_excl_scan_u32<NT>(fq_lane_lf(L), s_scan, &total);
    u64 bad = ~0ull;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j >= L.m) continue;
        const u32 c = L.c[j + 1];
        if (c == '\n') {
            if (idx < n_lf) lf[idx] = L.at + (u64)j;
            idx++;
        } else if ((c == ' ' || c == '\t') && (idx & 3) == 1 && bad == ~0ull) {
            bad = idx >> 2;
        }
    }
    if (bad != ~0ull) atomicMin((unsigned long long *)&aux[AUX_BAD_GROUP], (unsigned long long)bad);
    if (virt && blockIdx.x == 0 && tid == 0) lf[n_lf] = n_bytes;
}

// group j = lines 4 j .. 4 j + 3, all of them in the table (the last may end at the end of the text)
__global__ __launch_bounds__(NT) void fq_group_kernel(const u8 *text, u64 n_bytes, const u64 *lf, u64 n_groups, u64 *slen, u64 *hdr, u64 *aux) {
    const u64 j = (u64)blockIdx.x * NT + threadIdx.x;
    if (j == n_groups) slen[j] = 0;
    if (j >= n_groups) return;
    const u64 s0 = j ? lf[4 * j - 1] + 1 : 0;
    const u64 e0 = lf[4 * j], e1 = lf[4 * j + 1], e2 = lf[4 * j + 2], e3 = lf[4 * j + 3];
    bool ok = text[s0] == '@';                          // 1. a line that begins with '@' (an empty one begins with its LF)
    u64 sl = e1 - e0 - 1;
    if (sl && text[e0 + 1] == '+') ok = false;          // 2. the sequence line does not begin with '+' (blanks: fq_table_kernel)
    if (sl && text[e1 - 1] == '\r') sl--;
    if (text[e1 + 1] != '+') ok = false;                // 3. a line that begins with '+'
    u64 ql = e3 - e2 - 1;
    if (ql && e3 < n_bytes && text[e3 - 1] == '\r') ql--;  // (a CR at the end of the text is not in front of an LF)
    if (ql < sl) ok = false;                            // 4. the quality line covers the sequence
    slen[j] = sl;
    hdr[j] = s0;
    if (!ok) atomicMin((unsigned long long *)&aux[AUX_BAD_GROUP], (unsigned long long)j);
}

// res[0] = the groups in front of the first bad one, res[1] = their bases, res[2] = the byte behind them
__global__ void fq_result_kernel(const u64 *aux, const u64 *lf, const u64 *roff, u64 n_groups, u64 n_bytes, u64 *res) {
    const u64 bad = aux[AUX_BAD_GROUP];
    const u64 good = bad < n_groups ? bad : n_groups;
    u64 end = good ? lf[4 * good - 1] + 1 : 0;
    if (end > n_bytes) end = n_bytes;
    res[0] = good;
    res[1] = roff[good];
    res[2] = end;
}

__global__ __launch_bounds__(NT) void fq_write_kernel(const u8 *text, u64 n_bytes, const u64 *loffs, const u64 *lf, const u64 *roff, u64 good,
                                                      u8 *out_bases) {
    __shared__ uint4 s_img[FX_IMG / 16];
    __shared__ uint4 s_out[FX_IMG / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    __shared__ u64 s_dest;
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * FASTX_TILE;
    const u8 *B = fx_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    FxLane L;
    fx_lane(B, n_bytes, start, tid, L);
    u32 total;
    const u64 idx0 = loffs[blockIdx.x] + (u64)block_excl_scan_u32<NT>(fq_lane_lf(L), s_scan, &total);
    u64 idx = idx0;
    u32 kept = 0;
    int first = -1;  // the lane's first kept byte
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j >= L.m) continue;
        const u32 c = L.c[j + 1];
        if (c == '\n') {
            idx++;
        } else if ((idx & 3) == 1 && (idx >> 2) < good && !(c == '\r' && L.c[j + 2] == '\n')) {
            if (first < 0) first = j;
            kept++;
        }
    }
    const u32 excl = block_excl_scan_u32<NT>(kept, s_scan, &total);
    if (total == 0) return;
    if (kept && excl == 0) {  // the tile's first kept byte: byte (its position - the start of its line) of record g
        u64 i1 = idx0;
#pragma unroll
        for (int j = 0; j < FX_VT; j++) i1 += (j < first && L.c[j + 1] == '\n') ? 1u : 0u;
        const u64 g = i1 >> 2;
        s_dest = roff[g] + (L.at + (u64)first - (lf[4 * g] + 1));
    }
    __syncthreads();
    u8 *dst = out_bases + s_dest;
    int shift;
    u8 *O = image_at(dst, s_out, &shift);
    u32 k = excl;
    idx = idx0;
#pragma unroll
    for (int j = 0; j < FX_VT; j++) {
        if (j >= L.m) continue;
        const u32 c = L.c[j + 1];
        if (c == '\n') idx++;
        else if ((idx & 3) == 1 && (idx >> 2) < good && !(c == '\r' && L.c[j + 2] == '\n')) O[k++] = (u8)c;
    }
    __syncthreads();
    flush_image(dst, total, s_out, shift, tid);
}

struct FxOut {
    u8 *bases;
    u64 bases_cap;
    u64 *rec_off, *hdr_off;
    u64 rec_cap;
    u64 *n_bases, *n_rec, *n_consumed;
    int *stop;
};
// the sizes are known: *n_bases / *n_rec / *n_consumed / *stop, then UKM_ERR_CAPACITY where either array is too small
int fx_sizes(const char *name, const FxOut &o, u64 nb, u64 nr, u64 consumed, int stop) {
    *o.n_bases = nb;
    *o.n_rec = nr;
    *o.n_consumed = consumed;
    *o.stop = stop;
    if (o.rec_cap < nr)
        UKM_FAIL(UKM_ERR_CAPACITY, "%s: the text holds %llu records (%llu bases), rec_cap is %llu", name, (unsigned long long)nr,
                 (unsigned long long)nb, (unsigned long long)o.rec_cap);
    u64 unused;
    return out_fits(name, "the records hold", "bases", nb, o.bases_cap, &unused);
}
// a result without records: rec_off[0] = 0 is all there is to write
int fx_no_records(ukm_ctx *ctx, const FxOut &o) {
    if (!o.rec_off) return UKM_OK;
    u64 *ro = nullptr;
    UKM_TRY(ukm_out_t(ctx, o.rec_off, 1, &ro));
    UKM_HIP(hipMemsetAsync(ro, 0, sizeof(u64), ctx->stream));
    return UKM_OK;
}

int fasta_run(ukm_ctx *ctx, const char *name, const u8 *text, u64 n_bytes, bool last, const FxOut &o) {
    const u64 ntiles = (n_bytes + FASTX_TILE - 1) / FASTX_TILE;
    const dim3 grid((unsigned)ntiles), block(NT);
    u32 *tsum = nullptr;
    u64 *aux = nullptr;
    UKM_TRY(ws_alloc_t(ctx, ntiles, &tsum));
    UKM_TRY(ws_alloc_t(ctx, AUX_WORDS, &aux));
    SizeScan zr, zb;  // header lines, kept bytes
    UKM_TRY(size_alloc(ctx, ntiles, -1, &zr));
    UKM_TRY(size_alloc(ctx, ntiles, -1, &zb));
    UKM_HIP(hipMemsetAsync(aux, 0xFF, 2 * sizeof(u64), ctx->stream));
    UKM_HIP(hipMemsetAsync(aux + 2, 0, 2 * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(fa_summary_kernel, grid, block, 0, ctx->stream, text, n_bytes, tsum, zr.sums, aux);
    hipLaunchKernelGGL(fa_state_kernel, dim3(1), block, 0, ctx->stream, tsum, ntiles);
    hipLaunchKernelGGL(fa_tile_kernel<false>, grid, block, 0, ctx->stream, text, n_bytes, last ? 1 : 0, (const u32 *)tsum, aux, zb.sums,
                       (const u64 *)nullptr, (const u64 *)nullptr, (u8 *)nullptr, (u64 *)nullptr, (u64 *)nullptr, (u64)0, (u64)0, 0);
    UKM_HIP(hipGetLastError());
    UKM_TRY(size_scan(ctx, ntiles, &zr));
    UKM_TRY(size_scan(ctx, ntiles, &zb));
    u64 a[3];
    UKM_TRY(ukm_read_u64(ctx, aux, a, 3));
    const u64 H = zr.total;
    if (a[AUX_GARBAGE] < a[AUX_FIRST_HDR]) {  // (no header: ~0) the host dies there with its "invalid FASTA/Q format"
        UKM_TRY(fx_sizes(name, o, 0, 0, a[AUX_GARBAGE], UKM_FASTX_STOP_GRAMMAR));
        return fx_no_records(ctx, o);
    }
    u64 n_rec = H, consumed = n_bytes;
    int stop = UKM_FASTX_STOP_NONE;
    if (!last) {  // up to the start of the last header line
        n_rec = H ? H - 1 : 0;
        consumed = H ? a[AUX_LAST_HDR1] - 1 : 0;
        stop = UKM_FASTX_STOP_TAIL;
    }
    const u64 n_bases = zb.total;
    UKM_TRY(fx_sizes(name, o, n_bases, n_rec, consumed, stop));
    if (!o.rec_off) return UKM_OK;  // (the size query of a text without records)
    u8 *ob = nullptr;
    u64 *ro = nullptr, *ho = nullptr;
    if (n_bases) UKM_TRY(ukm_out_t(ctx, o.bases, n_bases, &ob));
    UKM_TRY(ukm_out_t(ctx, o.rec_off, n_rec + 1, &ro));
    if (o.hdr_off && n_rec) UKM_TRY(ukm_out_t(ctx, o.hdr_off, n_rec, &ho));
    write_begins(ctx);
    hipLaunchKernelGGL(fa_tile_kernel<true>, grid, block, 0, ctx->stream, text, n_bytes, last ? 1 : 0, (const u32 *)tsum, aux, (u32 *)nullptr,
                       (const u64 *)zb.offs, (const u64 *)zr.offs, ob, ro, ho, n_rec, n_bases, (last || H == 0) ? 1 : 0);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

int fastq_run(ukm_ctx *ctx, const char *name, const u8 *text, u64 n_bytes, bool last, const FxOut &o) {
    const u64 ntiles = (n_bytes + FASTX_TILE - 1) / FASTX_TILE;
    const dim3 block(NT);
    SizeScan zl;  // line ends
    UKM_TRY(size_alloc(ctx, ntiles, 0, &zl));
    hipLaunchKernelGGL(fq_count_kernel, dim3((unsigned)ntiles), block, 0, ctx->stream, text, n_bytes, zl.sums, zl.ctl);
    UKM_TRY(size_scan(ctx, ntiles, &zl));
    // with LAST the end of the text ends a line that lacks its LF; without, only lines that end in an LF count
    const bool virt = last && zl.flag != 0;
    const u64 n_lf = zl.total, n_lines = n_lf + (virt ? 1 : 0), G = n_lines / 4;
    if (G == 0) {  // not one group of four lines: the text is a tail, or (LAST) the host parser's
        UKM_TRY(fx_sizes(name, o, 0, 0, 0, last ? UKM_FASTX_STOP_GRAMMAR : UKM_FASTX_STOP_TAIL));
        return fx_no_records(ctx, o);
    }
    if ((G + NT) / NT > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call", name, (unsigned long long)G);
    u64 *lf = nullptr, *slen = nullptr, *roff = nullptr, *hdr = nullptr, *aux = nullptr;
    UKM_TRY(ws_alloc_t(ctx, n_lines, &lf));
    UKM_TRY(ws_alloc_t(ctx, G + 1, &slen));
    UKM_TRY(ws_alloc_t(ctx, G + 1, &roff));
    UKM_TRY(ws_alloc_t(ctx, G, &hdr));
    UKM_TRY(ws_alloc_t(ctx, 2 * AUX_WORDS, &aux));
    UKM_HIP(hipMemsetAsync(aux, 0xFF, sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(fq_table_kernel, dim3((unsigned)ntiles), block, 0, ctx->stream, text, n_bytes, (const u64 *)zl.offs, n_lf, virt ? 1 : 0, lf, aux);
    hipLaunchKernelGGL(fq_group_kernel, dim3((unsigned)((G + NT) / NT)), block, 0, ctx->stream, text, n_bytes, (const u64 *)lf, G, slen, hdr, aux);
    UKM_HIP(hipGetLastError());
    UKM_TRY(ukm_dev_exclusive_scan_u64(ctx, slen, roff, G + 1, nullptr));
    u64 *res = aux + AUX_WORDS;
    hipLaunchKernelGGL(fq_result_kernel, dim3(1), dim3(1), 0, ctx->stream, (const u64 *)aux, (const u64 *)lf, (const u64 *)roff, G, n_bytes, res);
    UKM_HIP(hipGetLastError());
    u64 r[3];
    UKM_TRY(ukm_read_u64(ctx, res, r, 3));
    const u64 good = r[0], n_bases = r[1], consumed = r[2];
    // a group that breaks a rule, or (LAST) lines that are no group: the host parser's, from the state it is in at a header
    const int stop = good < G ? UKM_FASTX_STOP_GRAMMAR
                     : consumed == n_bytes ? UKM_FASTX_STOP_NONE
                     : last ? UKM_FASTX_STOP_GRAMMAR : UKM_FASTX_STOP_TAIL;
    UKM_TRY(fx_sizes(name, o, n_bases, good, consumed, stop));
    if (!o.rec_off) return UKM_OK;
    if (good == 0) return fx_no_records(ctx, o);
    u8 *ob = nullptr;
    u64 *ro = nullptr, *ho = nullptr;
    if (n_bases) UKM_TRY(ukm_out_t(ctx, o.bases, n_bases, &ob));
    UKM_TRY(ukm_out_t(ctx, o.rec_off, good + 1, &ro));
    if (o.hdr_off) UKM_TRY(ukm_out_t(ctx, o.hdr_off, good, &ho));
    write_begins(ctx);
    if (n_bases) {
        const u64 wtiles = (consumed + FASTX_TILE - 1) / FASTX_TILE;
        hipLaunchKernelGGL(fq_write_kernel, dim3((unsigned)wtiles), block, 0, ctx->stream, text, n_bytes, (const u64 *)zl.offs, (const u64 *)lf,
                           (const u64 *)roff, good, ob);
        UKM_HIP(hipGetLastError());
    }
    UKM_HIP(hipMemcpyAsync(ro, roff, (good + 1) * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    if (ho) UKM_HIP(hipMemcpyAsync(ho, hdr, good * sizeof(u64), hipMemcpyDeviceToDevice, ctx->stream));
    return UKM_OK;
}

}  // namespace

extern "C" int ukm_fastx(ukm_ctx *ctx, const uint8_t *text, uint64_t n_bytes, uint32_t flags, uint8_t *out_bases, uint64_t bases_cap,
                         uint64_t *out_rec_off, uint64_t *out_hdr_off, uint64_t rec_cap, uint64_t *n_bases, uint64_t *n_rec,
                         uint64_t *n_consumed, int *stop) {
    const char *name = "ukm_fastx";
    if (!ctx || !n_bases || !n_rec || !n_consumed || !stop || (!text && n_bytes) || (!out_bases && bases_cap) || (!out_rec_off && rec_cap))
        UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_bases = *n_rec = *n_consumed = 0;
    *stop = UKM_FASTX_STOP_NONE;
    if (flags & ~(UKM_FASTX_FASTQ | UKM_FASTX_LAST)) UKM_FAIL(UKM_ERR_INVALID, "%s: unknown flags %u", name, flags);
    if ((n_bytes + FASTX_TILE - 1) / FASTX_TILE > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu bytes in one call", name, (unsigned long long)n_bytes);
    if (n_bytes == 0 && !out_rec_off) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const FxOut o = {out_bases, bases_cap, out_rec_off, out_hdr_off, rec_cap, n_bases, n_rec, n_consumed, stop};
        if (n_bytes == 0) return fx_no_records(ctx, o);
        const u8 *b = nullptr;
        UKM_TRY(ukm_in_t(ctx, text, n_bytes, &b));
        const bool last = (flags & UKM_FASTX_LAST) != 0;
        return (flags & UKM_FASTX_FASTQ) ? fastq_run(ctx, name, b, n_bytes, last, o) : fasta_run(ctx, name, b, n_bytes, last, o);
    }();
    return ukm_finish(&s, rc);
}
