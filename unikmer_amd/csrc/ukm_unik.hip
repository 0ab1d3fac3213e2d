// ukm_unik.hip — ukm_unik_decode / ukm_unik_encode: the body of a `.unik` file (everything behind the header, inflated)
// to and from arrays of codes and taxids.  The byte layout is the one host/unik.hpp states (unik::Reader::read,
// unik::Writer::write_code_with_taxid / flush); the calls are held to it byte for byte.
//
// Fixed-size layouts (unsorted, compact): a record is cb + tb bytes, one kernel per direction, a tile of FIX_RECS records
// staged through LDS.
//
// Sorted layout, decode.  Record boundaries depend on the data: a pair is 1 + l0 + l1 + 2 tb bytes, a single 9 + tb, at
// most REC_MAX = 25.  The body is cut into tiles of DEC_TILE bytes.  The first record that STARTS inside a tile begins at
// one of NENT = 25 entry offsets (0..24), so a tile is a function entry offset -> (exit offset = the next tile's entry,
// codes counted, delta sum mod 2^64, "a single reset the sum", "a record ran past the end of the body").  These maps
// compose associatively:
//   1. summary_kernel: per tile, the bytes plus a 24-byte tail go to LDS as aligned 16-byte words (no word that lies
//      wholly outside the body is loaded, bytes outside it are never looked at); every position is decoded in parallel as
//      if a record started there (length, delta sum); 25 lanes walk their chains and leave the tile's map.
//   2. group_map_kernel: one workgroup composes the maps of SCAN_GROUP consecutive tiles, 25 lanes, maps staged through
//      LDS SCAN_CHUNK at a time.  chain_kernel with one workgroup then follows the TRUE chain over the groups (entry 0,
//      code index 0, prev 0): the number of codes and the error bit of the whole body come out here, so the size query
//      and a capacity failure end before any output pass.  chain_kernel over the groups' tiles leaves every tile's true
//      (entry offset, code index, prev).
//   3. decode_kernel: per tile the same LDS image and per-position decode, one lane lists the tile's records with their
//      code index and prev, all threads write codes and taxids, record i by thread i.
// No look-back: a carried prev needs all 64 bits, and a map is no sum.  Chains are never assumed to merge.
//
// Sorted layout, encode: size-then-write (ukm_bytes.h: SizeScan).  enc_sum_kernel adds the byte lengths of ENC_PAIRS pairs
// per tile (and raises the flag word where the Writer refuses the order), enc_write_kernel builds a tile's bytes in LDS and
// writes them as aligned 16-byte words with a head and a tail of single bytes.  Both take a thread's deltas and their bytes
// from enc_load.  The decode's capacity step and bracket are the protocol's too; its chain is its own.
// load_image / flush_image / image_at, the byte helpers and the protocol: ukm_bytes.h (shared with ukm_text.hip, ukm_deflate.hip).
#include <algorithm>

#include "ukm_bytes.h"

namespace {

constexpr int DEC_TILE = 2048;   // body bytes per decode tile
constexpr int REC_MAX = 25;      // longest record: 1 + 8 + 8 + 2 * 4
constexpr int TAIL = REC_MAX - 1;
constexpr int NENT = REC_MAX;    // entry offsets 0..24
constexpr int DEC_IMG = DEC_TILE + TAIL + 24;      // + up to 15 bytes of alignment shift, rounded to 16
constexpr int DEC_MAXREC = DEC_TILE / 3 + 2;       // a pair is at least 3 bytes
constexpr int SCAN_GROUP = 256;  // tiles one scan workgroup composes
constexpr int SCAN_CHUNK = 64;   // maps in LDS at a time
constexpr int FIX_RECS = 1024;   // records per tile of the fixed-size layouts
constexpr int FIX_IMG = FIX_RECS * 12 + 32;
constexpr int ENC_PAIRS = 1024;  // pairs per tile of the sorted encode
constexpr int ENC_VT = ENC_PAIRS / NT;
constexpr int ENC_IMG = ENC_PAIRS * REC_MAX + 32;
static_assert(DEC_IMG % 16 == 0 && FIX_IMG % 16 == 0 && ENC_IMG % 16 == 0, "LDS images are whole 16-byte words");

enum : u32 { M_LEN = 31, M_SINGLE = 32, M_ERR = 64 };  // per-position meta byte
enum : u32 { EX_OFF = 255, EX_RESET = 256, EX_ERR = 512 };
enum : u32 { ST_RESET = 1, ST_ERR = 2 };

struct TileMap {  // one entry offset of one tile (or group of tiles)
    u64 sum;      // delta sum behind the last reset
    u32 n;        // codes
    u32 ex;       // exit offset | EX_RESET | EX_ERR
};
static_assert(sizeof(TileMap) == 16, "maps are moved as 16-byte words");

struct WalkState {  // the true chain in front of a tile (or group)
    u64 prev;
    u64 n;      // codes in front
    u32 off;    // entry offset
    u32 flags;  // ST_*
};

// every position p < npos of a tile as if a record started there; `remaining` = body bytes from the tile's start on
__device__ inline void precompute(const u8 *B, u32 npos, u64 remaining, int tb, u8 *meta, u64 *val, int tid) {
    for (u32 p = (u32)tid; p < npos; p += NT) {
        const u32 ctrl = B[p];
        u32 m;
        u64 v = 0;
        if (ctrl & 128u) {
            const u32 len = 9u + (u32)tb;
            if ((u64)p + len > remaining) m = M_ERR;
            else {
                v = get_be(B + p + 1, 8);
                m = len | M_SINGLE;
            }
        } else {
            const int l0 = (int)((ctrl >> 3) & 7u) + 1, l1 = (int)(ctrl & 7u) + 1;
            const u32 len = 1u + (u32)l0 + (u32)l1 + 2u * (u32)tb;
            if ((u64)p + len > remaining) m = M_ERR;
            else {
                v = get_be(B + p + 1, l0) + get_be(B + p + 1 + l0, l1);
                m = len;
            }
        }
        meta[p] = (u8)m;
        val[p] = v;
    }
}

__global__ __launch_bounds__(NT) void summary_kernel(const u8 *body, u64 n_bytes, int tb, TileMap *maps) {
    __shared__ uint4 s_img[DEC_IMG / 16];
    __shared__ u64 s_val[DEC_TILE];
    __shared__ u8 s_meta[DEC_TILE];
    const int tid = (int)threadIdx.x;
    const u64 tile = blockIdx.x, start = tile * (u64)DEC_TILE, remaining = n_bytes - start;
    const u32 len = (u32)(remaining < (u64)(DEC_TILE + TAIL) ? remaining : (u64)(DEC_TILE + TAIL));
    const u32 npos = len < (u32)DEC_TILE ? len : (u32)DEC_TILE;
    const int shift = load_image(body, start, len, s_img, tid);
    __syncthreads();
    precompute((const u8 *)s_img + shift, npos, remaining, tb, s_meta, s_val, tid);
    __syncthreads();
    if (tid >= NENT) return;
    u32 pos = (u32)tid, n = 0, ex = 0;
    u64 sum = 0;
    while (pos < npos) {
        const u32 m = s_meta[pos];
        if (m & M_ERR) {
            ex |= EX_ERR;
            break;
        }
        const u64 v = s_val[pos];
        if (m & M_SINGLE) {
            sum = v;
            ex |= EX_RESET;
            n += 1;
        } else {
            sum += v;
            n += 2;
        }
        pos += m & M_LEN;
    }
    if (!(ex & EX_ERR) && pos >= (u32)DEC_TILE) ex |= pos - (u32)DEC_TILE;
    TileMap t;
    t.sum = sum;
    t.n = n;
    t.ex = ex;
    maps[tile * NENT + (u64)tid] = t;
}

// lanes tid < lanes each follow a chain over maps[first .. first + count); out_states (lane 0's chain): the state in
// front of every map.  All threads of the workgroup call this together.
__device__ inline void walk_maps(const TileMap *maps, u64 first, u64 count, int lanes, WalkState &st, WalkState *out_states,
                                 TileMap *s_chunk, int tid) {
    for (u64 c0 = 0; c0 < count; c0 += SCAN_CHUNK) {
        const u32 m = (u32)(count - c0 < (u64)SCAN_CHUNK ? count - c0 : (u64)SCAN_CHUNK);
        const uint4 *src = (const uint4 *)(maps + (first + c0) * NENT);
        for (u32 i = (u32)tid; i < m * NENT; i += NT) ((uint4 *)s_chunk)[i] = src[i];
        __syncthreads();
        if (tid < lanes) {
            for (u32 j = 0; j < m; j++) {
                if (out_states && tid == 0) out_states[first + c0 + j] = st;
                if (st.flags & ST_ERR) continue;
                const TileMap t = s_chunk[j * NENT + st.off];
                st.n += t.n;
                if (t.ex & EX_RESET) {
                    st.prev = t.sum;
                    st.flags |= ST_RESET;
                } else {
                    st.prev += t.sum;
                }
                st.off = t.ex & EX_OFF;
                if (t.ex & EX_ERR) st.flags |= ST_ERR;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void group_map_kernel(const TileMap *maps, u64 ntiles, TileMap *gmaps) {
    __shared__ uint4 s_chunk[SCAN_CHUNK * NENT];
    const int tid = (int)threadIdx.x;
    const u64 first = (u64)blockIdx.x * SCAN_GROUP;
    const u64 count = ntiles - first < (u64)SCAN_GROUP ? ntiles - first : (u64)SCAN_GROUP;
    WalkState st;
    st.prev = 0;
    st.n = 0;
    st.off = tid < NENT ? (u32)tid : 0u;
    st.flags = 0;
    walk_maps(maps, first, count, NENT, st, nullptr, (TileMap *)s_chunk, tid);
    if (tid < NENT) {
        TileMap t;
        t.sum = st.prev;
        t.n = (u32)st.n;  // at most SCAN_GROUP * (DEC_TILE / 3 + 1) * 2
        t.ex = st.off | ((st.flags & ST_RESET) ? EX_RESET : 0u) | ((st.flags & ST_ERR) ? EX_ERR : 0u);
        gmaps[(u64)blockIdx.x * NENT + (u64)tid] = t;
    }
}

// workgroup b follows the true chain over maps[b * per .. min((b + 1) * per, total)), from start[b] (null: the start of the
// body); result (null or two words): codes and error bit behind the last map
__global__ __launch_bounds__(NT) void chain_kernel(const TileMap *maps, u64 per, u64 total, const WalkState *start, WalkState *out_states,
                                                   u64 *result) {
    __shared__ uint4 s_chunk[SCAN_CHUNK * NENT];
    const int tid = (int)threadIdx.x;
    const u64 first = (u64)blockIdx.x * per;
    const u64 count = total - first < per ? total - first : per;
    WalkState st;
    st.prev = 0;
    st.n = 0;
    st.off = 0;
    st.flags = 0;
    if (start) st = start[blockIdx.x];
    walk_maps(maps, first, count, 1, st, out_states, (TileMap *)s_chunk, tid);
    if (result && tid == 0) {
        result[0] = st.n;
        result[1] = (st.flags & ST_ERR) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(NT) void decode_kernel(const u8 *body, u64 n_bytes, int tb, const WalkState *states, u64 *out_keys,
                                                    u32 *out_tax) {
    __shared__ uint4 s_img[DEC_IMG / 16];
    __shared__ u64 s_val[DEC_TILE];
    __shared__ u64 s_rprev[DEC_MAXREC];
    __shared__ unsigned short s_rpos[DEC_MAXREC], s_ridx[DEC_MAXREC];
    __shared__ u8 s_meta[DEC_TILE];
    __shared__ u32 s_nrec;
    const int tid = (int)threadIdx.x;
    const u64 tile = blockIdx.x, start = tile * (u64)DEC_TILE, remaining = n_bytes - start;
    const u32 len = (u32)(remaining < (u64)(DEC_TILE + TAIL) ? remaining : (u64)(DEC_TILE + TAIL));
    const u32 npos = len < (u32)DEC_TILE ? len : (u32)DEC_TILE;
    const int shift = load_image(body, start, len, s_img, tid);
    __syncthreads();
    const u8 *B = (const u8 *)s_img + shift;
    precompute(B, npos, remaining, tb, s_meta, s_val, tid);
    __syncthreads();
    const WalkState st = states[tile];
    if (tid == 0) {
        u32 pos = st.off, cnt = 0, i = 0;
        u64 prev = st.prev;
        while (pos < npos && i < (u32)DEC_MAXREC) {
            const u32 m = s_meta[pos];
            if (m & M_ERR) break;  // (the chain kernels have seen it: this launch does not happen then)
            s_rpos[i] = (unsigned short)pos;
            s_ridx[i] = (unsigned short)cnt;
            s_rprev[i] = prev;
            const u64 v = s_val[pos];
            if (m & M_SINGLE) {
                prev = v;
                cnt += 1;
            } else {
                prev += v;
                cnt += 2;
            }
            pos += m & M_LEN;
            i++;
        }
        s_nrec = i;
    }
    __syncthreads();
    const u32 nrec = s_nrec;
    for (u32 r = (u32)tid; r < nrec; r += NT) {
        const u32 p = s_rpos[r];
        const u64 o = st.n + s_ridx[r];
        const u32 ctrl = B[p];
        if (ctrl & 128u) {
            out_keys[o] = s_val[p];
            if (out_tax) out_tax[o] = (u32)get_be(B + p + 9, tb);
        } else {
            const int l0 = (int)((ctrl >> 3) & 7u) + 1, l1 = (int)(ctrl & 7u) + 1;
            const u64 pv = s_rprev[r];
            out_keys[o] = pv + get_be(B + p + 1, l0);
            out_keys[o + 1] = pv + s_val[p];
            if (out_tax) {
                out_tax[o] = (u32)get_be(B + p + 1 + l0 + l1, tb);
                out_tax[o + 1] = (u32)get_be(B + p + 1 + l0 + l1 + tb, tb);
            }
        }
    }
}

__global__ __launch_bounds__(NT) void fixed_decode_kernel(const u8 *body, u64 n, int cb, int tb, u64 *out_keys, u32 *out_tax) {
    __shared__ uint4 s_img[FIX_IMG / 16];
    const int tid = (int)threadIdx.x;
    const u64 r0 = (u64)blockIdx.x * FIX_RECS;
    const u32 m = (u32)(n - r0 < (u64)FIX_RECS ? n - r0 : (u64)FIX_RECS);
    const u32 R = (u32)(cb + tb);
    const int shift = load_image(body, r0 * R, m * R, s_img, tid);
    __syncthreads();
    const u8 *B = (const u8 *)s_img + shift;
    for (u32 r = (u32)tid; r < m; r += NT) {
        out_keys[r0 + r] = get_be(B + r * R, cb);
        if (out_tax) out_tax[r0 + r] = (u32)get_be(B + r * R + cb, tb);
    }
}

__global__ __launch_bounds__(NT) void fixed_encode_kernel(const u64 *keys, const u32 *tax, u64 n, int cb, int tb, u8 *out) {
    __shared__ uint4 s_img[FIX_IMG / 16];
    const int tid = (int)threadIdx.x;
    const u64 r0 = (u64)blockIdx.x * FIX_RECS;
    const u32 m = (u32)(n - r0 < (u64)FIX_RECS ? n - r0 : (u64)FIX_RECS);
    const u32 R = (u32)(cb + tb);
    u8 *dst = out + r0 * R;
    int shift;
    u8 *B = image_at(dst, s_img, &shift);
    for (u32 r = (u32)tid; r < m; r += NT) {
        put_be(B + r * R, keys[r0 + r], cb);
        if (tb) put_be(B + r * R + cb, tax ? tax[r0 + r] : 0u, tb);
    }
    __syncthreads();
    flush_image(dst, m * R, s_img, shift, tid);
}

// pair j of a sorted stream: its deltas, and whether the Writer refuses it
__device__ inline bool pair_deltas(const u64 *keys, u64 j, u64 *d0, u64 *d1) {
    const u64 prev = j ? keys[2 * j - 1] : 0, c0 = keys[2 * j], c1 = keys[2 * j + 1];
    *d0 = c0 - prev;
    *d1 = c1 - c0;
    return c0 < prev || c1 < c0;
}

// a thread's ENC_VT pairs from pair j0 on: their deltas (zeros behind pair npairs - 1), the bytes of their records, and
// *bad: the Writer refuses one of them
__device__ inline u32 enc_load(const u64 *keys, u64 npairs, int tb, u64 j0, u64 *d0, u64 *d1, bool *bad) {
    u32 bytes = 0;
    *bad = false;
    for (int s = 0; s < ENC_VT; s++) {
        d0[s] = d1[s] = 0;
        if (j0 + s >= npairs) continue;
        *bad |= pair_deltas(keys, j0 + s, &d0[s], &d1[s]);
        bytes += 1u + (u32)byte_len(d0[s]) + (u32)byte_len(d1[s]) + 2u * (u32)tb;
    }
    return bytes;
}

__global__ __launch_bounds__(NT) void enc_sum_kernel(const u64 *keys, u64 npairs, int tb, u32 *sums, u64 *ctl) {
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    u64 d0[ENC_VT], d1[ENC_VT];
    bool bad;
    const u32 bytes = enc_load(keys, npairs, tb, (u64)blockIdx.x * ENC_PAIRS + (u64)tid * ENC_VT, d0, d1, &bad);
    u32 total;
    (void)block_excl_scan_u32<NT>(bytes, s_scan, &total);
    if (tid == 0) sums[blockIdx.x] = total;
    if (bad) atomicOr((unsigned long long *)&ctl[1], 1ull);
}

__global__ __launch_bounds__(NT) void enc_write_kernel(const u64 *keys, const u32 *tax, u64 npairs, int tb, const u64 *offs, u8 *out) {
    __shared__ uint4 s_img[ENC_IMG / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 j0 = (u64)blockIdx.x * ENC_PAIRS + (u64)tid * ENC_VT;
    u64 d0[ENC_VT], d1[ENC_VT];
    bool bad;  // (the size pass has reported it: this launch does not happen then)
    const u32 bytes = enc_load(keys, npairs, tb, j0, d0, d1, &bad);
    u32 total;
    u32 at = block_excl_scan_u32<NT>(bytes, s_scan, &total);
    u8 *dst = out + offs[blockIdx.x];
    int shift;
    u8 *B = image_at(dst, s_img, &shift);
    for (int s = 0; s < ENC_VT; s++) {
        const u64 j = j0 + s;
        if (j >= npairs) break;
        const int l0 = byte_len(d0[s]), l1 = byte_len(d1[s]);
        B[at] = (u8)(((l0 - 1) << 3) | (l1 - 1));
        put_be(B + at + 1, d0[s], l0);
        put_be(B + at + 1 + l0, d1[s], l1);
        at += 1u + (u32)l0 + (u32)l1;
        if (tb) {
            put_be(B + at, tax ? tax[2 * j] : 0u, tb);
            put_be(B + at + tb, tax ? tax[2 * j + 1] : 0u, tb);
            at += 2u * (u32)tb;
        }
    }
    __syncthreads();
    flush_image(dst, total, s_img, shift, tid);
}

// the trailing record of an odd count: ctrl = 128, the full code, its taxid
__global__ void enc_single_kernel(const u64 *keys, const u32 *tax, u64 idx, int tb, u8 *dst) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u8 b[16];
    b[0] = 128;
    put_be(b + 1, keys[idx], 8);
    if (tb) put_be(b + 9, tax ? tax[idx] : 0u, tb);
    for (int i = 0; i < 9 + tb; i++) dst[i] = b[i];
}

// the layout the header fields describe: *cb = code bytes of a fixed-size record (0: sorted), *tb = taxid bytes (0: none)
int layout(const char *name, int k, uint32_t flags, int taxid_bytes, int *cb, int *tb) {
    *tb = 0;
    if (flags & UKM_UNIK_INCLUDE_TAXID) {
        if (taxid_bytes < 1 || taxid_bytes > 4) UKM_FAIL(UKM_ERR_INVALID, "%s: taxid_bytes = %d, must be 1..4", name, taxid_bytes);
        *tb = taxid_bytes;
    }
    if (flags & UKM_UNIK_SORTED) {
        *cb = 0;
    } else if (flags & UKM_UNIK_COMPACT) {
        if (k < 1 || k > 32) UKM_FAIL(UKM_ERR_K, "%s: k = %d, a compact body needs 1..32", name, k);
        *cb = (k + 3) / 4;
    } else {
        *cb = 8;
    }
    return UKM_OK;
}

}  // namespace

extern "C" uint64_t ukm_unik_encode_bound(uint64_t n, int k, uint32_t flags, int taxid_bytes) {
    const u64 tb = (flags & UKM_UNIK_INCLUDE_TAXID) ? (u64)std::min(std::max(taxid_bytes, 0), 4) : 0;
    if (flags & UKM_UNIK_SORTED) return (n / 2) * (17 + 2 * tb) + (n & 1) * (9 + tb);
    const u64 cb = (flags & UKM_UNIK_COMPACT) ? (u64)((std::min(std::max(k, 1), 32) + 3) / 4) : 8;
    return n * (cb + tb);
}

extern "C" int ukm_unik_decode(ukm_ctx *ctx, const uint8_t *body, uint64_t n_bytes, int k, uint32_t flags, int taxid_bytes,
                               uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_unik_decode";
    if (!ctx || !n_out || (!body && n_bytes) || (!out_keys && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    int cb = 0, tb = 0;
    UKM_TRY(layout(name, k, flags, taxid_bytes, &cb, &tb));
    if (n_bytes == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u8 *b = nullptr;
        u64 *ok = nullptr;
        u32 *ot = nullptr;
        if (cb) {  // fixed-size records
            const u64 R = (u64)(cb + tb), n = n_bytes / R, rest = n_bytes % R;
            if (rest) UKM_FAIL(UKM_ERR_FORMAT, "%s: %s: the last record holds %llu of %llu bytes", name,
                               rest < (u64)cb ? "truncated record" : "unexpected EOF", (unsigned long long)rest, (unsigned long long)R);
            UKM_TRY(out_fits(name, "the body holds", "records", n, out_cap, n_out));
            const u64 nblocks = (n + FIX_RECS - 1) / FIX_RECS;
            if (nblocks > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call", name, (unsigned long long)n);
            UKM_TRY(ukm_in_t(ctx, body, n_bytes, &b));
            UKM_TRY(ukm_out_t(ctx, out_keys, n, &ok));
            if (tb) UKM_TRY(ukm_out_t(ctx, out_taxids, n, &ot));
            hipLaunchKernelGGL(fixed_decode_kernel, dim3((unsigned)nblocks), dim3(NT), 0, ctx->stream, b, n, cb, tb, ok, ot);
            UKM_HIP(hipGetLastError());
            return UKM_OK;
        }
        const u64 ntiles = (n_bytes + DEC_TILE - 1) / DEC_TILE, ngroups = (ntiles + SCAN_GROUP - 1) / SCAN_GROUP;
        if (ntiles > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu bytes in one call", name, (unsigned long long)n_bytes);
        UKM_TRY(ukm_in_t(ctx, body, n_bytes, &b));
        TileMap *maps = nullptr, *gmaps = nullptr;
        WalkState *tstates = nullptr, *gstates = nullptr;
        u64 *result = nullptr;
        UKM_TRY(ws_alloc_t(ctx, ntiles * NENT, &maps));
        UKM_TRY(ws_alloc_t(ctx, ngroups * NENT, &gmaps));
        UKM_TRY(ws_alloc_t(ctx, ngroups, &gstates));
        UKM_TRY(ws_alloc_t(ctx, 2, &result));
        hipLaunchKernelGGL(summary_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, b, n_bytes, tb, maps);
        scan_begins(ctx);  // (the protocol's bracket around a scan of its own: a map is no sum)
        hipLaunchKernelGGL(group_map_kernel, dim3((unsigned)ngroups), dim3(NT), 0, ctx->stream, (const TileMap *)maps, ntiles, gmaps);
        hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(NT), 0, ctx->stream, (const TileMap *)gmaps, ngroups, ngroups,
                           (const WalkState *)nullptr, gstates, result);
        UKM_HIP(hipGetLastError());
        u64 res[2] = {0, 0};
        UKM_TRY(ukm_read_u64(ctx, result, res, 2));
        if (res[1]) UKM_FAIL(UKM_ERR_FORMAT, "%s: unexpected EOF: the last record runs past the body's %llu bytes", name,
                             (unsigned long long)n_bytes);
        UKM_TRY(out_fits(name, "the body holds", "records", res[0], out_cap, n_out));
        if (res[0] == 0) return UKM_OK;
        UKM_TRY(ws_alloc_t(ctx, ntiles, &tstates));
        UKM_TRY(ukm_out_t(ctx, out_keys, res[0], &ok));
        if (tb) UKM_TRY(ukm_out_t(ctx, out_taxids, res[0], &ot));
        hipLaunchKernelGGL(chain_kernel, dim3((unsigned)ngroups), dim3(NT), 0, ctx->stream, (const TileMap *)maps, (u64)SCAN_GROUP, ntiles,
                           (const WalkState *)gstates, tstates, (u64 *)nullptr);
        write_begins(ctx);
        hipLaunchKernelGGL(decode_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, b, n_bytes, tb, (const WalkState *)tstates, ok, ot);
        UKM_HIP(hipGetLastError());
        return UKM_OK;
    }();
    return ukm_finish(&s, rc);
}

extern "C" int ukm_unik_encode(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, int k, uint32_t flags,
                               int taxid_bytes, uint8_t *out_bytes, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_unik_encode";
    if (!ctx || !n_out || (!keys && n) || (!out_bytes && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    int cb = 0, tb = 0;
    UKM_TRY(layout(name, k, flags, taxid_bytes, &cb, &tb));
    if (n == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *dk = nullptr;
        const u32 *dt = nullptr;
        u8 *ob = nullptr;
        if (cb) {
            const u64 R = (u64)(cb + tb), need = n * R;
            UKM_TRY(out_fits(name, "the body takes", "bytes", need, out_cap, n_out));
            const u64 nblocks = (n + FIX_RECS - 1) / FIX_RECS;
            if (nblocks > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call", name, (unsigned long long)n);
            UKM_TRY(ukm_in_t(ctx, keys, n, &dk));
            if (tb) UKM_TRY(ukm_in_t(ctx, taxids, n, &dt));
            UKM_TRY(ukm_out_t(ctx, out_bytes, need, &ob));
            hipLaunchKernelGGL(fixed_encode_kernel, dim3((unsigned)nblocks), dim3(NT), 0, ctx->stream, dk, dt, n, cb, tb, ob);
            UKM_HIP(hipGetLastError());
            return UKM_OK;
        }
        const u64 npairs = n / 2, ntiles = (npairs + ENC_PAIRS - 1) / ENC_PAIRS;
        if (ntiles > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call", name, (unsigned long long)n);
        UKM_TRY(ukm_in_t(ctx, keys, n, &dk));
        if (tb) UKM_TRY(ukm_in_t(ctx, taxids, n, &dt));
        SizeScan z;  // of the pairs: z.total stays 0 without one
        if (npairs) {
            UKM_TRY(size_alloc(ctx, ntiles, 0, &z));  // the flag: a pair out of order
            hipLaunchKernelGGL(enc_sum_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, dk, npairs, tb, z.sums, z.ctl);
            UKM_TRY(size_scan(ctx, ntiles, &z));
            if (z.flag) UKM_FAIL(UKM_ERR_UNSORTED, "%s: codes written to a sorted .unik must be ascending", name);
        }
        const u64 need = z.total + (n & 1) * (u64)(9 + tb);
        UKM_TRY(out_fits(name, "the body takes", "bytes", need, out_cap, n_out));
        UKM_TRY(ukm_out_t(ctx, out_bytes, need, &ob));
        if (npairs) {
            write_begins(ctx);
            hipLaunchKernelGGL(enc_write_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, dk, dt, npairs, tb, (const u64 *)z.offs, ob);
        }
        if (n & 1) hipLaunchKernelGGL(enc_single_kernel, dim3(1), dim3(64), 0, ctx->stream, dk, dt, n - 1, tb, ob + z.total);
        UKM_HIP(hipGetLastError());
        return UKM_OK;
    }();
    return ukm_finish(&s, rc);
}
