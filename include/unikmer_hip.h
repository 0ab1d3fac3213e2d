/*
 * unikmer_hip.h — C ABI of libunikmer_hip.so, the MI355X (gfx950) implementation of the
 * k-mer encode / ntHash / sort / set-operation hot path of shenwei356/unikmer v0.21.0.
 *
 * The reference has no FFI; the seam is the Go package API of its third-party modules plus
 * a few in-tree loops.  Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference/unikmer/cmd/).  INTEGRATION.md
 * shows the cgo binding a maintainer would add on the Go side.
 *
 * Conventions
 *  - Every call returns int: 0 = UKM_OK, negative = error class; the message is available
 *    through ukm_last_error() (thread-local).  Nothing here ever calls exit()/abort()
 *    (the reference's checkError -> os.Exit(-1), util-cli.go:39-44, stays on the Go side).
 *  - Array arguments may be HOST or DEVICE pointers, independently per argument
 *    (hipPointerGetAttributes decides).  Device pointers are used in place; host arrays are
 *    staged through the context's device workspace.  Scalar outputs (n_out) are host
 *    pointers.  All buffers are caller-owned; nothing is retained after the call returns
 *    (cgo pointer-passing rules), except the taxonomy which is copied into the context.
 *  - Alignment: a device pointer needs only the natural alignment of its element type -- 8 bytes for codes, offsets and
 *    uint64 outputs, 4 for taxids, 1 for bases and uint8 outputs -- so streams may be sub-allocated back to back from one
 *    slab.  Results never depend on the address.  A call reads nothing as data, and writes nothing, outside the arrays it
 *    was given: whatever lies in front of or behind an array (a neighbour's records included) has no influence on the
 *    result and is left as it was.
 *  - Outputs are caller-allocated with capacity `out_cap` (elements); upper bounds:
 *    union <= sum(n), inter <= n[0], diff <= n[0], common <= sum(n), unique <= n (2n for
 *    UKM_REPEATED_CHUNK), encode/nthash <= number of windows.  Too small -> UKM_ERR_CAPACITY.
 *    Size query: with out_cap == 0 every output pointer may be NULL (out_taxids too, also for records that carry taxids); the
 *    call returns UKM_ERR_CAPACITY with the size needed in *n_out, or UKM_OK with *n_out == 0 for an empty result.  A failed
 *    call leaves [0, out_cap) unspecified; nothing outside [0, out_cap) is ever written.
 *  - A ukm_ctx owns one HIP stream and one growable device workspace; it is NOT thread-safe.
 *    Use one ctx per calling OS thread (the reference calls these seams from several
 *    goroutines: sort.go:257, diff.go:280).  There is no global mutable state.
 *  - Records are (code uint64, taxid uint32) in structure-of-arrays form (kmers.go:24-27 is
 *    the AoS Go struct).  `taxids == NULL` means "no taxid information".
 *  - Sorted inputs are required where the reference requires the sorted flag
 *    (inter.go:139-141, diff.go:115-117); the library verifies sortedness on the fly where
 *    that is free and returns UKM_ERR_UNSORTED.
 */
#ifndef UNIKMER_HIP_H
#define UNIKMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UKM_OK 0
#define UKM_ERR_INVALID (-1)      /* bad argument */
#define UKM_ERR_HIP (-2)          /* HIP runtime failure (message has the hipError string) */
#define UKM_ERR_NOMEM (-3)        /* device or host allocation failed */
#define UKM_ERR_ILLEGAL_BASE (-4) /* kmers.ErrIllegalBase: a window contains a non-IUPAC byte */
#define UKM_ERR_UNSORTED (-5)     /* an input that must be sorted is not */
#define UKM_ERR_NO_TAXONOMY (-6)  /* taxids present but ukm_taxonomy_load was not called */
#define UKM_ERR_CAPACITY (-7)     /* out_cap too small; *n_out holds the required size */
#define UKM_ERR_K (-8)            /* k out of range (1..32 codes, 1..64 hashes; count.go:81-87) */
#define UKM_ERR_PEER (-9)         /* a collective call: another rank reported a failure; no rank went on (see that rank) */
#define UKM_ERR_FORMAT (-10)      /* a .unik body ends inside a record (unik.hpp: "truncated record", "unexpected EOF"); a line outside ukm_dump's grammar */

/* scan / merge modes: sort.go:484-572 (-u / -d / plain), util-sort.go:35-190 (chunk protocol) */
#define UKM_PLAIN 0
#define UKM_UNIQUE 1
#define UKM_REPEATED 2
#define UKM_REPEATED_CHUNK 3
#define UKM_SINGLETON 4      /* codes seen exactly once: `count -u` (count.go:424-432,475-486) */

/* 2-way set operations */
#define UKM_OP_UNION 0
#define UKM_OP_INTER 1
#define UKM_OP_DIFF 2

/* flags */
#define UKM_F_MIX_TAXID 2u   /* inter --mix-taxid, inter.go:229-236 */
#define UKM_F_CMP_TAXID 4u   /* diff -t/--compare-taxid, diff.go:361-362,406-407 */
#define UKM_F_INVERT 8u      /* grep -v / filter -v: keep the records the predicate rejects */
#define UKM_F_QUERY_TAXID 16u /* grep -t: the queries are taxids (kept for symmetry: a non-NULL q_taxids already says so) */
#define UKM_F_DEVICE_STREAMS 256u /* n-way calls (union / inter / diff / common): every keys[i] / taxids[i] is a DEVICE pointer.
                                   * Without it each pointer is classified with hipPointerGetAttributes (host arrays are
                                   * staged), which for a fold over 1000 files is 2000 driver queries = most of the call's
                                   * host time.  A host that keeps decoded .unik streams on the device sets it. */

typedef struct ukm_ctx ukm_ctx;

/* ---- library / context -------------------------------------------------------------- */
const char *ukm_last_error(void);
int ukm_version(void);                       /* 1000*major + minor */
int ukm_device_count(int *n);
int ukm_ctx_create(int device, ukm_ctx **out);
int ukm_ctx_destroy(ukm_ctx *ctx);
/* borrow a caller's hipStream_t (e.g. the framework's current stream) instead of the ctx's own
 * non-blocking stream; NULL is HIP's default (null) stream.  Work the caller enqueued on that
 * stream before a ukm_* call is ordered before the call's kernels. */
int ukm_ctx_set_stream(ukm_ctx *ctx, void *hip_stream);
int ukm_ctx_sync(ukm_ctx *ctx);
/* pre-size the device workspace so that later calls do not allocate */
int ukm_ctx_reserve(ukm_ctx *ctx, uint64_t bytes);
/* give the device workspace back to the driver (it grows to what the largest call needed and is kept for the next one:
 * a 100-file union of 1e10 records leaves 160 GB behind); the next call allocates again */
int ukm_ctx_trim(ukm_ctx *ctx);
/* device-memory helpers for hosts without their own allocator (the cgo shim) */
int ukm_dev_alloc(ukm_ctx *ctx, uint64_t bytes, void **dptr);
int ukm_dev_free(ukm_ctx *ctx, void *dptr);
int ukm_copy(ukm_ctx *ctx, void *dst, const void *src, uint64_t bytes); /* any direction, synchronous */
/* Streaming uploads / downloads (the host side of count.go:285-299: FASTA/Q is read in chunks while the device
 * works on the previous chunk).  ukm_host_alloc gives page-locked host memory; ukm_copy_async enqueues a copy
 * (any direction) on the context's TRANSFER stream and returns at once: it starts after the compute work the
 * context was given before the call and then runs beside later compute calls.  ukm_copy_fence orders every
 * LATER compute call behind the transfers issued so far (device-side wait, the host does not block);
 * ukm_copy_sync blocks the host until they are done (before a host source buffer is reused or a host
 * destination is read).  Double buffering: copy_async(chunk i+1) ; compute(chunk i) ; copy_fence ; ... */
int ukm_host_alloc(ukm_ctx *ctx, uint64_t bytes, void **hptr);
int ukm_host_free(ukm_ctx *ctx, void *hptr);
int ukm_copy_async(ukm_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int ukm_copy_fence(ukm_ctx *ctx);
int ukm_copy_sync(ukm_ctx *ctx);
/* ms between hipEvents recorded on the ctx stream (a) around the DOMINANT kernel of the most
 * recent compute call (the tiled set-op kernel for ukm_setop2; falls back to (b) when a call
 * records none) and (b) around all device work of the call */
int ukm_last_kernel_ms(ukm_ctx *ctx, float *ms);
int ukm_last_call_ms(ukm_ctx *ctx, float *ms);
/* diagnostic: which internal route answered the most recent n-way call (ukm_union / ukm_merge_k / ukm_common), one of
 * UKM_ROUTE_*.  Tests use it to see that a knob took effect. */
#define UKM_ROUTE_NONE 0     /* none / 2-way only */
#define UKM_ROUTE_TREE 1     /* pairwise tree of 2-way kernels */
#define UKM_ROUTE_KWAY 2     /* multi-level k-way streaming merge */
#define UKM_ROUTE_PUNION 3   /* LDS hash-probe union */
#define UKM_ROUTE_SRMERGE 4  /* single-pass range merge (one LDS tile per value range) */
#define UKM_ROUTE_SRCOMMON 5 /* the same pass counting the records of every code (ukm_common below the number of files) */
#define UKM_ROUTE_PCOMMON 6  /* ukm_common / ukm_merge_k -d by counting hash probes */
#define UKM_ROUTE_PLACE 7    /* keep-everything merge by placement (counts per code, runs written in one piece) */
int ukm_last_route(ukm_ctx *ctx);

/* ---- route policy as API (round 5).  The n-way entry points choose between several internal routes (ukm_last_route) by
 *      the shape of their inputs; the thresholds can be overridden PER CONTEXT:
 *        ukm_ctx_set_option(ctx, key, value) / ukm_ctx_unset_option / ukm_ctx_get_option (is_set = 0: the library decides).
 *      Keys a host may care about (value semantics as the UKM_<KEY> developer variables of DESIGN.md 4.12):
 *        "punion"  0 never take the hash-probe union / counting probes, 1 whenever the shape allows (size thresholds
 *                  ignored), 2 also without the hit-rate and load guards;   "punion_tax" 0: records with taxids never;
 *        "punion_ranked" 0: files with one taxid each go through the generic taxid tables;
 *        "place" 0 / 1 keep-everything merge by placement never / whenever possible;   "srmerge" 0 / 1 single-pass merge;
 *        "kway" 1 k-way merge also for tiny inputs;   "no_kway" 1 pairwise tree only;   "no_fold" / "no_pfold" 1 the
 *        one-launch range / probe folds of inter and diff off;   "pfold_tax" 0;   "common_probe" 0;   "sort_local" 0 all
 *        radix passes through HBM;   "win_strip" / "nthash_strip" 0 / 1;   "force_ticket" 1 dispatch-order independent kernels
 *        (a context whose look-back watchdog has fired keeps them whatever this option says);   "sort_counting" 0 digit
 *        passes inside every LDS bucket, "sort_fan" 0 no size-class fan-out;   "setop_src" 0 / 1 / 2 the two-launch source-word
 *        route of a 2-way operation with per-record taxids never / for inter / also for union (default: 0 on a taxonomy
 *        with one-byte clade codes, else 1);   "setop_defer" 0 the LCAs of a 2-way union / inter with per-record taxids inside the
 *        merge step instead of densely behind it;   "punion_clade" / "srmerge_clade" 0 / 1
 *        clade codes in the probe tables / the single pass's emit never / always;
 *        "grep_lds" 0 / 1 ukm_grep by codes: the queries never / whenever they fit (2048 of them) in an LDS table per
 *        workgroup instead of sorted behind a prefix directory.
 *      Developer / test keys: "ws_poison" b (0..255) fills the whole device workspace with byte b before every
 *        call, so that a kernel reading a workspace word it never initialised cannot pass by luck; unset: nothing is enqueued.
 *      The environment is read ONCE, when a context is created: every UKM_* variable present then is the context's default
 *      for the matching key; no compute call calls getenv (a context created under UKM_ENV_LIVE=1 -- the test suite, which
 *      flips knobs between calls -- keeps looking).  An explicitly set option always wins.
 *      ukm_ctx_get_stat: "punion_attempts" = base sets the last hash-probe union / counting-probe call built (2: its retry
 *      with four times the files ran), "workspace_bytes" = device workspace currently held by the context, "workspace_blocks" = the allocations it consists of,
 *      "ws_poisoned_bytes" = bytes option "ws_poison" has filled since the most recent call began (the blocks that call created, the
 *      block they were merged into when it ended and a later ukm_ctx_reserve included; the next call starts from zero), "sort_fused_hist" = sorts of this context whose first
 *      digit histogram came from the kernel that produced the keys (ukm_count) instead of a pass of their own, "grep_route" =
 *      the membership shape of the last ukm_grep (1 LDS table, 2 prefix directory, 3 taxid bitmap, 0 no kernel ran),
 *      "count_window_retries" = ukm_count calls of this context that ran their window pass twice (more windows passed the
 *      Scaled filter than the size estimate of the internal buffer allowed for; the second pass is sized exactly),
 *      "window_route" = the kernel that wrote the windows of the context's most recent window pass (ukm_encode_kmers, ukm_nthash,
 *      and the inner window pass of ukm_minimizer, ukm_count, ukm_locate and the map calls): 1 window_kernel (the general one),
 *      2 stripwin_kernel (rolling strips, long records), 3 nthash_strip_kernel (rolling strips behind the Scaled filter).  It is
 *      set to 0 when such a pass begins, so a pass that ends before any launch (no record, no window) shows 0,
 *      "window_strip_declined" = launches of a strip kernel, over the context's life, that gave up -- more records under one
 *      tile than stripwin_kernel's table holds, more candidates in one tile than nthash_strip_kernel's list -- so that the
 *      general kernel answered the call (same result, one wasted launch),
 *      "sort_route" = the route that completed the context's most recent outermost radix sort (ukm_sort_u64, ukm_sort_pairs
 *      and the sort inside every call that sorts): 1 host histograms, 2 fused histograms, 3 top bits + LDS buckets, 4 chunks
 *      of 2^31 records merged (the sorts of the chunks, and of the oversized buckets gathered by route 3, do not overwrite it),
 *      "sort_bucket_declined" = times, over the context's life, route 3 was entered and handed the keys to the general passes
 *      (narrow keys, a sample or the bucket sizes said "crowded"), "sort_oversized_buckets" = buckets beyond the largest size
 *      class that the most recent outermost sort, if it took route 3, gathered and sorted by the general passes (0 when none; a
 *      route-4 sort leaves it as it was: the sorts of its chunks do not write it),
 *      "punion_flags" = the flag word the most recent hash-probe pass of this context left (union, union of files with one
 *      taxid each, counting probes of `common`; 0 when none has run, and cleared when a call tries such a route, so that
 *      an attempt that declines in front of its pass shows 0 and not an earlier call's word): 1 PU_FLAG_UNSORTED a file is not sorted, 2
 *      PU_FLAG_OVERFLOW the list of records the base set lacks outgrew its estimated size (stores are guarded), 4
 *      PU_FLAG_TAXID a taxid outside the loaded taxonomy, 8 PU_FLAG_RAW a record no table could take.  Any bit makes the
 *      route decline without having written the output, and the general merge answers the call.
 *      "setop_part_hits" = ukm_setop2 / ukm_setop2_ft calls of this context that took their merge-path table from the call
 *      before them on the same two device buffers (after verifying it against the buffers as they are now),
 *      "setop_part_stale" = such calls whose table failed the verification, so that the search ran after all (after two in
 *      a row the context stops trying),
 *      "setop_offs_hits" = of those hits, calls on plain codes (no taxids) whose pass also took the output offsets of its
 *      tiles from the match counts a call before it left with the table, and so ran without the look-back,
 *      "setop_offs_stale" = such calls whose tiles counted otherwise (contents rewritten in place under an unchanged
 *      partition): the pass ran again with the look-back (after two in a row the context stops trying).  See ukm_setop2.
 *      "setop_multi_fused" / "setop_multi_split" = ukm_setop2_multi calls of this context that were answered by the one
 *      fused pass / by one ordinary pass per operation (a call that began fused and met duplicate codes counts as split),
 *      "lb_watchdogs" = times a look-back watchdog fired in this context (a tile's predecessor did not publish: the
 *      launch was repeated with ticketed tile ids, or a chained inter / diff fold fell back to the synchronous fold),
 *      "ticket_latched" = 1 once that has happened: every later look-back kernel of the context takes its tile ids from
 *      tickets, for the context's lifetime (0 otherwise; option "force_ticket" does not show here),
 *      "inflate_candidates" / "inflate_segments" = of the last ukm_inflate: the offsets it found behind a marker 00 00 FF FF
 *      (offset 0 included), and how many of them began a segment on the chain: the rest were false hits;
 *      "inflate_cp_walk_us" = the device time, in microseconds, of that call's second walk over the chain (the checkpoints):
 *      the part of its write side that is not the write pass (0 where the call ended before it). */
int ukm_ctx_set_option(ukm_ctx *ctx, const char *key, long long value);
int ukm_ctx_unset_option(ukm_ctx *ctx, const char *key);
int ukm_ctx_get_option(ukm_ctx *ctx, const char *key, long long *value, int *is_set);
int ukm_ctx_get_stat(ukm_ctx *ctx, const char *key, unsigned long long *value);

/* ---- taxonomy: replaces taxdump.NewTaxonomyFromNCBI / LoadMergedNodesFromNCBI / LCA
 *      (util.go:119-171; 14 taxondb.LCA call sites).
 *      child/parent = the first two columns of nodes.dmp; merged_* = merged.dmp (may be NULL).
 *      Contract (taxdump parity is unpinned): LCA(0,x)=LCA(x,0)=0; LCA(x,x)=x;
 *      merged ids are remapped; ids absent from nodes.dmp -> 0.
 *      The device tables are dense in the taxid (>= 27 bytes per id up to the largest one, 16 more per id for every four
 *      levels of depth): NCBI's dump takes ~0.7 GB; a dump with sparse huge ids is refused (UKM_ERR_NOMEM, message says
 *      how much it would need) when that exceeds the device's free memory -- counted after the context's cached workspace
 *      has been given back and with the tables being replaced credited.  A load either replaces the context's taxonomy
 *      completely or, on any error, leaves the previous one in place (one exception: new tables that only fit WITHOUT the
 *      old ones make the old ones go first; a failure after that leaves the context without a taxonomy). */
int ukm_taxonomy_load(ukm_ctx *ctx, const uint32_t *child, const uint32_t *parent, uint64_t n,
                      const uint32_t *merged_old, const uint32_t *merged_new, uint64_t m);
int ukm_taxonomy_max_taxid(ukm_ctx *ctx, uint32_t *max_taxid); /* taxdump.MaxTaxid, util.go:169 */
int ukm_lca(ukm_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out);
/* rank of every node: rank_id[i] in 1..255 names the rank of child[i] (the host numbers the rank strings of
 * nodes.dmp's third column, lower-cased); 0 = this node has no known rank.  Needs a loaded taxonomy
 * (UKM_ERR_NO_TAXONOMY); a child that is not a node of it: UKM_ERR_INVALID, nothing changed.  Nodes the call does not
 * name keep rank id 0 (a second call replaces the whole column).  One byte per id on the device.
 * ukm_taxonomy_load drops the ranks together with the tables it replaces. */
int ukm_taxonomy_set_ranks(ukm_ctx *ctx, const uint32_t *child, const uint8_t *rank_id, uint64_t n);

/* ---- encode: replaces sketches.NewKmerIterator(seq,k,canonical,circular).NextKmer()
 *      (count.go:321,363) = kmers v0.1.0 2-bit encode + canonical.
 *      bases = concatenated records, rec_off[n_rec+1] = record boundaries.  Records shorter
 *      than k are skipped (sketches.ErrShortSeq, count.go:323-328).  Output = every window of
 *      every record in order. */
int ukm_encode_kmers(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off,
                     uint64_t n_rec, int k, int canonical, int circular, uint64_t *out,
                     uint64_t out_cap, uint64_t *n_out);

/* ---- ntHash: replaces sketches.NewHashIterator(...).NextHash() (count.go:319,361) and
 *      nthash.NewHasher(&seq,k).Next(canonical) (dump.go:253-260) = ntHash v1; fused with the
 *      Scaled-MinHash filter `code > maxHash -> skip` (count.go:98,373-375) when max_hash != 0.
 *      Output keeps window order. */
int ukm_nthash(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec,
               int k, int canonical, int circular, uint64_t max_hash, uint64_t *out,
               uint64_t out_cap, uint64_t *n_out);
/* ---- minimizer sketch: replaces sketches.NewMinimizerSketch(seq,k,w,circular).NextMinimizer()
 *      (count.go:316,357; bio v0.13.3, SURVEY.md B3, KATs C-7/C-8): canonical ntHash of every
 *      window; for each group of w consecutive windows of a record the LEFTMOST minimum, emitted
 *      when the arg-min position differs from the previous group's.  Records with fewer than w
 *      windows give nothing.  max_hash != 0 applies the Scaled filter to the emitted values
 *      (count.go:373-375).  out_pos (may be NULL) = window index of each minimizer inside its
 *      record (sketch.Index()).  1 <= w <= 1024.  Output keeps record/group order. */
int ukm_minimizer(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec,
                  int k, int w, int circular, uint64_t max_hash, uint64_t *out,
                  uint64_t *out_pos, uint64_t out_cap, uint64_t *n_out);
/* count.go:98  maxHash = uint64(float64(^uint64(0)) / float64(scale)) */
uint64_t ukm_max_hash(uint64_t scale);
/* ---- `count` in one call: replaces the body of the Run closure count.go:285-436 (iterator + `m[code] = struct{}{}` per
 *      k-mer, the -u / -d marks of count.go:424-432) and its sort count.go:581: every window of every record (codes when
 *      hashed = 0, ntHash v1 with the Scaled filter max_hash != 0 when hashed = 1) -> sort -> mode UKM_UNIQUE (the distinct
 *      set), UKM_REPEATED (`-d`: codes seen at least twice) or UKM_SINGLETON (`-u`: exactly once), sorted ascending (`-s`).
 *      The windows stay in the context's device workspace (8 B per base while the call runs); only the result is written to
 *      out[out_cap] (host or device).  The same result as ukm_encode_kmers / ukm_nthash + ukm_sort_u64 + ukm_unique with one
 *      stream synchronisation instead of three.  Too small an out_cap: UKM_ERR_CAPACITY, *n_out = the size needed.
 *      UKM_ERR_CAPACITY speaks about out_cap ONLY: out never needs more than the result's size, however many windows pass
 *      the filter.  The internal window buffer of a Scaled sketch is sized from an estimate; input that defeats it (a
 *      low-complexity record whose one hash lies below max_hash) costs a second window pass into a buffer of the exact
 *      size (stat "count_window_retries"), never an error. */
int ukm_count(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, int k, int canonical,
              int circular, int hashed, uint64_t max_hash, int mode, uint64_t *out, uint64_t out_cap, uint64_t *n_out);

/* ---- k-mers back to the genome: replace the bodies of `unikmer locate` (locate.go:141-289) and `unikmer map` / `uniqs`
 *      (map.go:116-491 at its default gap settings -x 0 -X 0).  Windows are always CANONICAL (both commands demand the
 *      canonical flag of their inputs): 2-bit codes when hashed = 0, ntHash v1 when hashed = 1.  bases / rec_off as for
 *      ukm_encode_kmers; records shorter than k contribute nothing; out_rec indexes the caller's records (skipped ones
 *      counted).  Errors as ukm_encode_kmers / ukm_nthash give them (UKM_ERR_K, UKM_ERR_ILLEGAL_BASE).  Limits: fewer than
 *      2^32 windows per call (window indices are the 32-bit payload of the pair sort; UKM_ERR_INVALID above that), fewer
 *      than 2^32 queries / set codes.
 *      ukm_locate: q_keys[nq] = the content of the .unik files in file order, neither sorted nor distinct.  Output: one
 *      entry per (query, window with that code), queries in q_keys order, each code only where it FIRST appears in q_keys
 *      (locate.go:284 `delete(m, code)`), a query's windows ascending by (record, position).  out_q = index into q_keys,
 *      out_pos = index of the window in its record (iter.Index()); with circular the windows are the circular iterator's,
 *      so out_pos + k may exceed the record length (the reference slices a record extended by its first k - 1 bases).
 *      Upper bound of the output: the number of windows.
 *      ukm_map: set_keys[n_set] sorted ascending (duplicates tolerated; UKM_ERR_UNSORTED otherwise); genome_off[n_genome + 1]
 *      groups consecutive records into genomes (genome_off[0] = 0, genome_off[n_genome] = n_rec).  A window is GOOD when its
 *      code is in the set and -- unless allow_multi -- occurs exactly once among the windows of its genome (map.go:252-257
 *      "multiple mapped").  Output: every maximal run of consecutive good windows inside one record with
 *      last - first + k >= min_len (min_len >= 1), as rec, start = first, end = last + k, in record then position order:
 *      what the state machine of map.go:362-489 emits at -x 0 -X 0.  Context option "map_sorted" (both calls): 0 the windows look
 *      their codes up in genome order, 1 all (code, window) pairs are sorted first; default: by the size of the set / the
 *      number of queries. */
int ukm_locate(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, int k, int circular, int hashed,
               const uint64_t *q_keys, uint64_t nq, uint64_t *out_q, uint32_t *out_rec, uint64_t *out_pos,
               uint64_t out_cap, uint64_t *n_out);
int ukm_map(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, const uint64_t *genome_off,
            uint64_t n_genome, int k, int hashed, const uint64_t *set_keys, uint64_t n_set, int allow_multi,
            uint64_t min_len, uint32_t *out_rec, uint64_t *out_start, uint64_t *out_end, uint64_t out_cap,
            uint64_t *n_out);

/* ---- ukm_map_gapped: `unikmer map` with -x / -X / --circular (map.go:298-490).  Arguments, contracts, errors and the
 *      option "map_sorted" are ukm_map's; max_gap_size = -x, max_gap_num = -X.  Per record of L >= k bases every window
 *      has one of three classes: G its code is in the set and (allow_multi, or it occurs once among the windows of its
 *      genome); B in the set but multiple-mapped (never with allow_multi); M not in the set.  Linear records: the STREAM is
 *      the record's L - k + 1 windows.  circular: the classes are those of the record's L circular windows (multiplicity is
 *      counted among exactly these, map.go:222-226) and the stream has 2L - k + 1 positions, position i with the class of
 *      circular window i mod L (the reference maps the record written twice, map.go:338-340).
 *        1. RUNS are the maximal stretches of G inside one record's stream.
 *        2. The separator in front of a run is SOFT when it consists of M only and is at most max_gap_size long; HARD when
 *           it contains a B, is longer, or the run is the first of its record.  A CHAIN is a maximal sequence of runs
 *           joined by soft separators.
 *        3. With the runs of a chain numbered from 0 and X = max_gap_num, a REGION is the group of runs
 *           [j(X + 1), j(X + 1) + X], cut at the chain's end: start = first window of the group's first run, last = last
 *           window of its last run.  The small gap behind a full group belongs to no region.
 *        4. A region is kept when last - start + k >= min_len.  Linear: (rec, start, last + k).  circular: regions with
 *           start >= L are dropped (map.go:407/423); the end is start + L when last - start + k > L (map.go:381), else
 *           last + k, and may exceed L.
 *        5. Output in record order, then start order.  max_gap_size = 0 ignores max_gap_num (the reference warns and
 *           ignores); max_gap_size = 0 with circular = 0 is exactly ukm_map.
 *      Two deliberate deviations from map.go: `flag`, `lastGapNum` and `lastmatch` start every
 *      record as they start the first one (the reference carries them over, and a record that ends inside a tolerated gap
 *      makes the next records lose every region up to their first hard break); after the circular `break` nothing more is
 *      emitted for the record (the reference prints a stale region shorter than k, visible only when min_len < k).
 *      UKM_ERR_INVALID: max_gap_size > 0 with max_gap_num = 0 (map.go:112); either gap value above 2^31 - 1; min_len < 1;
 *      2^31 or more stream positions in one call whenever gaps or circular are asked for (run and break counts share one
 *      look-back word): split the records over several calls.  UKM_ERR_CAPACITY: *n_out = the exact number of regions,
 *      nothing is written behind out_cap. */
int ukm_map_gapped(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, const uint64_t *genome_off,
                   uint64_t n_genome, int k, int hashed, int circular, const uint64_t *set_keys, uint64_t n_set,
                   int allow_multi, uint64_t min_len, uint64_t max_gap_size, uint64_t max_gap_num, uint32_t *out_rec,
                   uint64_t *out_start, uint64_t *out_end, uint64_t out_cap, uint64_t *n_out);

/* ---- sorts: replace sortutil.Uint64s (count.go:581, union.go:274,295, sort.go:463 ...) and
 *      sorts.Quicksort(CodeTaxidSlice) (sort.go:268,331,457).  In place, ascending by code;
 *      pairs are sorted by code only, stably.  key_bits = number of significant low bits
 *      (2k for k-mer codes, 0 or 64 for hashes): higher radix passes are skipped.
 *      Inputs of 2^32 records or more are sorted as 2^31-record chunks and merged on the
 *      device (the reference's own `sort -m` protocol, in HBM). */
int ukm_sort_u64(ukm_ctx *ctx, uint64_t *keys, uint64_t n, int key_bits);
int ukm_sort_pairs(ukm_ctx *ctx, uint64_t *keys, uint32_t *taxids, uint64_t n, int key_bits);

/* ---- scans over a sorted stream: replace sort.go:484-572 and dumpCodes2File /
 *      dumpCodesTaxids2File (util-sort.go:35-190).  taxids may be NULL. */
int ukm_unique(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n,
               int mode, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap,
               uint64_t *n_out);

/* ---- record selection: replace the record loops of `unikmer grep` (grep.go:617-676), `unikmer filter` (filter.go:130-151 with
 *      filterCode, filter.go:181-221) and `unikmer sample` (sample.go:134-148).  One predicate per record; the kept records are
 *      written in INPUT order, every duplicate included, each with its OWN taxid (copied, never folded: no taxonomy is needed).
 *      The input need not be sorted.  taxids == NULL: nothing is written to out_taxids.  Upper bound of the output: n.  Too small
 *      an out_cap: UKM_ERR_CAPACITY, *n_out = the size needed.  n == 0 is legal.  Outputs must not alias inputs.
 *      ukm_grep: exactly one of q_keys[nq] / q_taxids[nq] is non-NULL (both NULL only with nq == 0); the queries are neither
 *      sorted nor distinct.  q_keys: a record is kept when (its code is among q_keys) XOR UKM_F_INVERT; canonical_k in 1..32
 *      replaces every record's code by kmers.Canonical(code, k) before the lookup AND in the output (grep.go:641-643),
 *      canonical_k == 0 (hashed or canonical files) takes the codes as they are.  q_taxids: the test is on the record's taxid
 *      and the codes are written as they are (grep.go:628-633); with taxids == NULL every record carries file_taxid (what
 *      unik.Reader.ReadCodeWithTaxid hands out for a file with a global taxid), so the call is a copy or an empty result.
 *      nq == 0 keeps nothing; inverted, everything.  Fewer than 2^32 queries.
 *      ukm_filter: the low-complexity filter, exactly filterCode: bases are read from the LOW end of the code,
 *      scores[0] = penalty_d, scores[i] = penalty_s when base i equals base i - 1 else penalty_d; window > k is clamped to k;
 *      the sum of `window` scores is tested at positions 0 .. max(k - window - 1, 0) -- the last position, k - window, is never
 *      tested (filter.go:202) -- and a record is a HIT when some tested sum >= threshold.  Hits are dropped; with UKM_F_INVERT
 *      only hits are kept.  k in 1..64 (the hashed flag plays no part: bases above bit 63 read as 0, as Go's `code >>= 2`
 *      gives); penalties are plain ints, negative ones included; window >= 1, threshold >= 0.
 *      ukm_sample: keeps record j (1-based) when j >= start and (j - start) % window == 0; start >= 1, window >= 1. */
int ukm_grep(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint32_t file_taxid, uint64_t n,
             int canonical_k, const uint64_t *q_keys, const uint32_t *q_taxids, uint64_t nq, uint32_t flags,
             uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_filter(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, int k, int window,
               int penalty_s, int penalty_d, int threshold, uint32_t flags,
               uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_sample(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, uint64_t start,
               uint64_t window, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);

/* ---- filter by taxonomic rank: replaces newRankFilter + isPassed (rfilter.go:371-520) and the record loop of `unikmer rfilter`
 *      (rfilter.go:280-304).  The host reads the rank file (readRankOrderFromFile, rfilter.go:522-580), numbers the rank
 *      strings 1..255 (ukm_taxonomy_set_ranks) and states the filter in those numbers: */
typedef struct ukm_rank_filter {
    int32_t order[256];   /* > 0: rank id r is in the rank file's ordered list, larger = higher rank (the file's LAST
                             line has 1: rfilter.go:566-578); 0: r has no order ("!" ranks, rank id 0) */
    uint8_t no_rank[256]; /* 1: r is a "!" rank of the rank file */
    uint8_t black[256];   /* 1: r is on -B/--black-list */
    int32_t lower, higher;/* the ORDER of -L / -H, 0 = not given; both given: UKM_ERR_INVALID */
    int32_t equal[32]; int32_t n_equal;   /* the orders of -E */
    uint8_t discard_norank, save_norank, discard_root;  /* -N, -n, -R */
    uint32_t root_taxid;  /* --root-taxid */
} ukm_rank_filter;
/*      What happens to a record with taxid t -- isPassed as it is written, quirks included, in this order:
 *       1. discard_root and t == root_taxid: dropped.  The comparison is on the record's taxid as given.
 *       2. t at or beyond the table (above the largest id of the loaded dumps), t == 0, absent from the taxonomy, or of rank
 *          id 0: dropped (the reference's `Rank() == ""`).  A MERGED id is looked up as its target and a walk (6) starts
 *          from the target, as in ukm_lca; taxdump is not in the reference tree, so what its Rank does with a merged id is
 *          unpinned: this is the build's own contract.  Below, r = the rank id of t (of its target).
 *       3. black[r]: dropped.
 *       4. no_rank[r] and discard_norank: without save_norank dropped; with save_norank and lower != 0 the WALK (6) decides;
 *          with save_norank and lower == 0 the record goes on to 5 (newRankFilter does not refuse that, only the command
 *          line does).
 *       5. o = order[r] (0 for a rank without order; order[0] is never looked at).  o among equal[0 .. n_equal): kept.
 *          Otherwise with lower: kept when o < lower -- so a rank without order that 4 did not discard passes under -L; with
 *          higher: kept when o > higher; with neither: kept only when n_equal == 0.
 *       6. WALK (rfilter.go:469-491): p = parent[t]; then repeatedly: p == 1 (the literal 1 of the reference, not
 *          root_taxid, and tested BEFORE p's own rank is looked at): dropped; p absent: dropped; order[rank of p] > 0: kept
 *          when that order is <= lower (not <), dropped otherwise; parent[p] == p: dropped; else p = parent[p].  The two
 *          drops at an absent node and at a root other than 1 stand where the reference would loop for ever; wherever the
 *          reference terminates the results are the same.
 *      A record's fate depends on its taxid alone: one kernel over the taxonomy writes one keep bit per taxid (once per
 *      call), and the selection kernel of ukm_grep by taxid reads that bitmap.
 *      ukm_rank_filter_plan: 1-5 as a pure host function (no context, no device): what a taxid of rank r meets, as two
 *      256-byte tables.  self_action[r]: 0 dropped, 1 kept, 2 decided by the walk.  walk_action[r] for an ancestor of rank r:
 *      0 go on, 1 kept, 2 dropped.  lower and higher both non-zero, or n_equal outside 0..32: UKM_ERR_INVALID.
 *      ukm_rank_pass: out[i] = 1 when a record with taxids[i] is kept, else 0.  Host or device pointers, as ukm_lca.
 *      ukm_rfilter: the conventions of ukm_grep by taxid -- input order, duplicates kept, each record with its own taxid;
 *      taxids == NULL: every record carries file_taxid (a copy or an empty result); the size query and UKM_ERR_CAPACITY as
 *      everywhere.  Both need a taxonomy WITH ranks: UKM_ERR_NO_TAXONOMY otherwise. */
int ukm_rank_filter_plan(const ukm_rank_filter *f, uint8_t self_action[256], uint8_t walk_action[256]);
int ukm_rank_pass(ukm_ctx *ctx, const ukm_rank_filter *f, const uint32_t *taxids, uint64_t n, uint8_t *out);
int ukm_rfilter(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint32_t file_taxid, uint64_t n,
                const ukm_rank_filter *f, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);

/* ---- split by taxid: replaces the map of `unikmer tsplit` (tsplit.go:112-192): the records grouped by taxid, groups in
 *      ASCENDING taxid order (the reference's order is Go's map order, i.e. none), inside a group the codes in INPUT order
 *      (stable).  taxids[n] is required (a host with a file that has one global taxid needs no call).  out_keys[out_cap]:
 *      needs n.  group_taxids[group_cap], group_off[group_cap + 1]: group g is out_keys[group_off[g] .. group_off[g + 1]),
 *      group_off[n_groups] = n.  out_cap < n or group_cap < the number of groups: UKM_ERR_CAPACITY, *n_groups = the number
 *      of groups, nothing outside the capacities written; out_cap == 0 && group_cap == 0 is the size query (outputs may be
 *      NULL).  n == 0: UKM_OK, 0 groups, group_off untouched.  n >= 2^32: UKM_ERR_INVALID (record indices are the sort's
 *      32-bit payload).  No taxonomy is needed: taxids are plain numbers here, 0 and 2^32 - 1 included. */
int ukm_tsplit(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, uint64_t *out_keys, uint64_t out_cap,
               uint32_t *group_taxids, uint64_t *group_off, uint64_t group_cap, uint64_t *n_groups);

/* ---- .unik bodies: replace the record loops around unik.Reader.ReadCodeWithTaxid (union.go:187, inter.go:190 ...) and
 *      unik.Writer.WriteCode / WriteCodeWithTaxid / Flush.  The byte layout is the one unikmer_amd/host/unik.hpp states; both
 *      calls are held to that file byte for byte.  They take the BODY of a file: everything behind the header, already
 *      inflated; header parsing and gzip stay with the host.  k, flags and taxid_bytes are the header's own fields; of
 *      flags only the three bits below are looked at (SORTED wins over COMPACT, as in the Reader).  taxid_bytes: 1..4 with
 *      UKM_UNIK_INCLUDE_TAXID (UKM_ERR_INVALID otherwise), ignored without.  k: used by a compact unsorted body only, 1..32
 *      there (UKM_ERR_K).
 *      decode: out_keys / out_taxids [out_cap] receive what unik::Reader::read returns, record by record: a control byte
 *      with bit 7 set is one full 8-byte code wherever it stands and resets prev; bit 6 of a pair's control byte is ignored;
 *      prev + delta wraps mod 2^64; an unsorted record is (k + 3) / 4 bytes when compact, else 8, then taxid_bytes.  A body on
 *      which the Reader throws (it ends inside a record) gives UKM_ERR_FORMAT.  out_taxids == NULL is allowed also when the
 *      records carry taxids (they are skipped).  *n_out = the number of records; too small an out_cap (the size query
 *      included): UKM_ERR_CAPACITY with that number, and no output pass has run.
 *      encode: out_bytes[0, *n_out) is what unik::Writer puts behind the header for the same records, the trailing
 *      ctrl = 128 record of an odd count included; codes of a compact body and taxids are cut to their low bytes; taxids ==
 *      NULL with UKM_UNIK_INCLUDE_TAXID writes zeros.  With UKM_UNIK_SORTED: UKM_ERR_UNSORTED exactly where the Writer throws (a
 *      pair whose first code is below the previous pair's second, or whose second is below its first; equal codes are fine,
 *      and the trailing single is not looked at).  out_cap and *n_out are in BYTES; the size query and UKM_ERR_CAPACITY as
 *      everywhere.  The bound function is pure host code: exact for the fixed-size layouts, (n / 2) * (17 + 2 tb) +
 *      (n & 1) * (9 + tb) for a sorted body.
 *      body and out_bytes need no alignment.  Neither call uses the decoupled look-back: a carried code needs all 64 bits.
 *      After a call on a sorted body ukm_last_kernel_ms reports the scan between the two passes over the data (its launches
 *      and the read-back of the size), ukm_last_call_ms the whole call. */
#define UKM_UNIK_COMPACT 1u
#define UKM_UNIK_SORTED 4u
#define UKM_UNIK_INCLUDE_TAXID 8u
int ukm_unik_decode(ukm_ctx *ctx, const uint8_t *body, uint64_t n_bytes, int k, uint32_t flags, int taxid_bytes,
                    uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_unik_encode(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, int k, uint32_t flags,
                    int taxid_bytes, uint8_t *out_bytes, uint64_t out_cap, uint64_t *n_out);
uint64_t ukm_unik_encode_bound(uint64_t n, int k, uint32_t flags, int taxid_bytes);

/* ---- deflate: replace the gzip writer behind a .unik body (util-io.go:57-64, pgzip).  src [n_bytes] (host or device, any
 *      alignment) becomes a byte-aligned sequence of RFC 1951 blocks, none of them final unless asked: the source is cut into
 *      independent chunks of 32768 bytes, each one dynamic-Huffman block of literals followed by an empty stored block (the
 *      sync-flush marker), or one stored block where that would not be smaller.  No matches are searched for: a sorted body is
 *      delta bytes in which LZ77 finds nothing; k-mer TEXT is three times larger this way than through zlib and does not
 *      belong here.  Fragments concatenate: the caller's stream may hold zlib's own sync-flushed output in front of one.
 *      *crc32 is in/out: on entry the CRC-32 of the bytes that precede src in the caller's stream (0: none), on exit (UKM_OK
 *      only) the CRC-32 of those bytes followed by src.  *n_out = the fragment's bytes; out == NULL with out_cap == 0 is the
 *      size query; too small an out_cap: UKM_ERR_CAPACITY with the need, and nothing has been written to out.  Nothing
 *      outside out[0, *n_out) is ever written.  The output is a pure function of src and flags.  n_bytes == 0: an empty
 *      fragment, or just what the flags add.  UKM_DEFLATE_GZIP with *crc32 != 0 on entry: UKM_ERR_INVALID.
 *      ukm_deflate_bound (pure host code, never exceeded): n_bytes + 5 per chunk, + 2 with FINAL, + 20 with GZIP.
 *      ukm_crc32_combine (pure host code): the CRC-32 of A followed by B from crc(A), crc(B) and B's length, as zlib's
 *      crc32_combine; the library does not link zlib.
 *      After a call ukm_last_kernel_ms reports the scan between the two passes over the data (its launches and the two
 *      read-backs), ukm_last_call_ms the whole call. */
#define UKM_DEFLATE_FINAL 1u /* append the final empty block: the fragment then ends the deflate stream */
#define UKM_DEFLATE_GZIP 2u  /* implies FINAL: 10-byte gzip header in front, CRC-32 and ISIZE behind: a complete member */
int ukm_deflate(ukm_ctx *ctx, const uint8_t *src, uint64_t n_bytes, uint32_t flags, uint8_t *out, uint64_t out_cap,
                uint64_t *n_out, uint32_t *crc32);
uint64_t ukm_deflate_bound(uint64_t n_bytes, uint32_t flags);
uint32_t ukm_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---- inflate: read back what ukm_deflate wrote (and what zlib writes under Z_HUFFMAN_ONLY with a flush per chunk) without
 *      one host thread.  src [n_bytes] (host or device, any alignment) is a raw RFC 1951 fragment that starts at a block
 *      boundary on a byte boundary: the caller has taken off the gzip header, the trailer and anything in front.  The call
 *      inflates the longest prefix it understands and says where it stopped; the caller goes on from there with zlib
 *      (inflateSetDictionary with the last 32 KiB of output).
 *      It understands NON-FINAL blocks of all three types -- stored (at any bit position), fixed and dynamic Huffman --
 *      whose symbols are literals and end-of-block only.  It stops IN FRONT OF the first block that has BFINAL = 1 (even an
 *      empty one), has BTYPE = 11, contains a length symbol (257 or above), has LEN != ~NLEN, has an over-subscribed or
 *      incomplete code where zlib refuses that, or runs past n_bytes.  None of these is an error: the device never judges a
 *      stream, zlib meets the same block next and reports it in its own words.
 *      *n_consumed is always a block start on a byte boundary: offset 0, the byte behind a stored block that began on a byte
 *      boundary, or the byte behind an empty stored block (the marker 00 00 FF FF); a run of bit-packed blocks counts only
 *      as a whole, up to the empty stored block that closes it.  *n_out is the inflated size of exactly
 *      src[0, *n_consumed).  *n_consumed == 0 with *n_out == 0 is UKM_OK: that is what a zlib level-6 stream gives.
 *      *crc32 is in/out as in ukm_deflate: on entry the CRC-32 of the bytes in front of `out` in the caller's stream, on
 *      exit (UKM_OK only) the CRC-32 of those bytes followed by out[0, *n_out).
 *      out == NULL with out_cap == 0 is the size query; too small an out_cap: UKM_ERR_CAPACITY with the need in *n_out,
 *      *n_consumed set, and nothing has been written to out.  Nothing outside out[0, *n_out) is ever written.  The output
 *      is a pure function of src.  n_bytes == 0: UKM_OK, nothing consumed.  flags must be 0.
 *      ukm_inflate_bound (pure host code): 8 * n_bytes, a literal costs at least one bit -- a worst case that nobody
 *      should allocate: ask for the size, or take it from the gzip trailer.
 *      Limits: a marker-to-marker segment that inflates to 2^31 bytes or more ends the device's part in front of the block
 *      that crosses that size, and so do 256 consecutive segments that inflate to 2^32 bytes together; only long runs of
 *      stored blocks get there.  A segment is decoded by one lane, so it also ends in front of the block that takes it beyond
 *      2^20 literals of Huffman blocks or beyond 2^20 blocks: a Huffman-only stream that never flushes is zlib's from there.
 *      After a call ukm_last_kernel_ms reports the step between the size side and the write side (the scan over the
 *      chain's sizes and its read-back), ukm_last_call_ms the whole call. */
int ukm_inflate(ukm_ctx *ctx, const uint8_t *src, uint64_t n_bytes, uint32_t flags, uint8_t *out, uint64_t out_cap,
                uint64_t *n_out, uint64_t *n_consumed, uint32_t *crc32);
uint64_t ukm_inflate_bound(uint64_t n_bytes);

/* ---- k-mer text: replace the record loop of view.go:163-218 (everything except -g) and the line loop of dump.go:128-315
 *      (the paths that do not hash).  Byte buffers need no alignment; out_cap and *n_out of ukm_view are in BYTES; the size
 *      query, UKM_ERR_CAPACITY (with the exact size, and no output pass has run) and n == 0 / n_bytes == 0 as everywhere.
 *      view: the text `unikmer view` prints for the records, line by line.  The fields of a line: C = the code as an unsigned
 *      decimal without padding; T = the record's taxid, the same way (taxids == NULL: every record carries file_taxid, as in
 *      ukm_grep); K = with hashed == 0 k letters, letter i from the left "ACGT"[(code >> 2(k-1-i)) & 3] (bits above 2k are
 *      ignored), with hashed != 0 the same as C; Q = k times 'g', also when hashed.  k: 1..32 when hashed == 0, 1..64
 *      otherwise (UKM_ERR_K).  An unknown format, or UKM_VIEW_WITH_TAXID on a format other than FASTA / FASTQ: UKM_ERR_INVALID.
 *      ukm_view_bound is pure host code: exact for UKM_VIEW_KMER with hashed == 0, n (k + 1); else the worst case of 20 and
 *      10 digits.  All offsets are 64-bit (1e8 FASTA records are more than 4 GB).
 *      dump: the records of k-mer text, in line order.  The grammar is strict.  A line is the bytes between two LF, the
 *      last may lack its LF; one trailing CR is dropped; an empty line gives no record; every other line is field1 or, with
 *      UKM_DUMP_TAXID, field1 TAB field2, and nothing else.  field1: exactly k bytes, k in 1..32 (UKM_ERR_K), each one of
 *      A N M V H R D W (-> 0), C S B Y (-> 1), G K (-> 2), T U (-> 3) in either case; with UKM_DUMP_DECIMAL 1..20 digits with a
 *      value <= 2^64 - 1.  field2: 1..10 digits with a value <= 2^32 - 1.  A line that does not fit (a wrong length, another
 *      byte, a space, a TAB without the flag, none with it, a second TAB, a sign, too many digits, an overflow) gives
 *      UKM_ERR_FORMAT, and *bad_off (may be NULL; written in this case only) is the byte offset at which the first such line
 *      starts.  That is decided in the counting pass: it wins over UKM_ERR_CAPACITY.  UKM_DUMP_CANONICAL: code -> min(code,
 *      revcomp(code, k)); UKM_DUMP_CANONICAL_ONLY (wins over the former): a line whose code is not its own canonical form
 *      gives no record; either with UKM_DUMP_DECIMAL: UKM_ERR_INVALID.  out_taxids may be NULL: the second column is still
 *      checked, but not stored.  The number of LF + 1 bounds the number of records.
 *      After either call ukm_last_kernel_ms reports the scan between the two passes over the data (its launches and the
 *      read-back of the size), ukm_last_call_ms the whole call; the fixed-width view has one pass and no scan. */
#define UKM_VIEW_KMER 0u         /* K\n            view     */
#define UKM_VIEW_KMER_CODE 1u    /* K\tC\n         view -n  */
#define UKM_VIEW_CODE 2u         /* C\n            view -N  */
#define UKM_VIEW_KMER_TAXID 3u   /* K\tT\n         view -t  */
#define UKM_VIEW_TAXID 4u        /* T\n            view -T  */
#define UKM_VIEW_FASTA 5u        /* >C\nK\n        view -a  */
#define UKM_VIEW_FASTQ 6u        /* @C\nK\n+\nQ\n  view -q  */
#define UKM_VIEW_WITH_TAXID 16u  /* FASTA / FASTQ only: the header line is ">C T" / "@C T" (view -a -t, -q -t) */
int ukm_view(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint32_t file_taxid, uint64_t n, int k, int hashed,
             uint32_t format, uint8_t *out_bytes, uint64_t out_cap, uint64_t *n_out);
uint64_t ukm_view_bound(uint64_t n, int k, int hashed, uint32_t format);
#define UKM_DUMP_TAXID 1u          /* two columns: field1 TAB taxid */
#define UKM_DUMP_DECIMAL 2u        /* field1 is a decimal uint64 (dump --hashed); k is ignored */
#define UKM_DUMP_CANONICAL 4u      /* dump -K */
#define UKM_DUMP_CANONICAL_ONLY 8u /* dump -O */
int ukm_dump(ukm_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int k, uint32_t flags, uint64_t *out_keys,
             uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out, uint64_t *bad_off);

/* ---- FASTA/Q text: replace the byte loop of the sequence reader (bio/seqio/fastx as count.go:289-299 uses it; this
 *      project's statement of it is host/seqtext.hpp: parse_fastx, and the call is held to it byte for byte).  text [n_bytes]
 *      (host or device, any alignment) starts at a record boundary: the start of a file, or where an earlier call's
 *      *n_consumed pointed.  The call handles the longest prefix inside the device's grammar and says where it stopped; it
 *      never judges a file: what deviates is met by the host parser next and reported in its words.  It produces what a
 *      FastxSink sees for text[0, *n_consumed): out_bases = the kept sequence bytes, concatenated; out_rec_off[i] and
 *      out_rec_off[i + 1] bound record i there (out_rec_off[0] = 0, out_rec_off[*n_rec] = *n_bases; empty records are kept);
 *      out_hdr_off[i] (may be NULL) = the offset in text of record i's '>' or '@': the caller reads the name from the text it
 *      holds.  A line is the bytes between two LF.  A CR is dropped exactly when the next byte is an LF.  Space and TAB
 *      inside sequence lines are dropped; every other byte of a sequence line is copied as it stands (the encode kernels
 *      judge illegal bases).
 *      FASTA: a line whose first byte is '>' opens a record; every other line adds to the open record.  In front of the first
 *      header empty lines are skipped; any other line there stops the call: UKM_FASTX_STOP_GRAMMAR, *n_consumed = the start
 *      of that line, *n_rec = 0.  Without UKM_FASTX_LAST the call consumes up to the start of the last header line and
 *      returns UKM_FASTX_STOP_TAIL (*n_consumed == 0 where one record is longer than the text: call again with more).
 *      FASTQ (UKM_FASTX_FASTQ; the CALLER decides, as parse_fastx does: FASTQ iff the first line of the FILE is non-empty
 *      and begins with '@'): groups of exactly four lines from offset 0 -- a line that begins with '@'; a sequence line that
 *      does not begin with '+' and holds no blank (it may be empty); a line that begins with '+'; a quality line at least as
 *      long as the sequence line, both without their CR.  The first group that breaks a rule stops the call:
 *      UKM_FASTX_STOP_GRAMMAR, *n_consumed = that group's first byte, where the host's state machine expects a header.
 *      Without UKM_FASTX_LAST only groups whose four lines end in LF are consumed (UKM_FASTX_STOP_TAIL where bytes remain);
 *      with it the last quality line may lack its LF, and lines behind the last whole group are a UKM_FASTX_STOP_GRAMMAR.
 *      out_bases == NULL with bases_cap == 0 and rec_cap == 0 is the size query; either capacity too small:
 *      UKM_ERR_CAPACITY with both needs in *n_bases / *n_rec, *n_consumed and *stop set, and nothing written.  Nothing outside
 *      out_bases[0, *n_bases), out_rec_off[0, *n_rec] and out_hdr_off[0, *n_rec) is ever written.  n_bytes == 0: UKM_OK,
 *      nothing consumed, UKM_FASTX_STOP_NONE.  Unknown flag bits: UKM_ERR_INVALID.  The output is a pure function of text and
 *      flags.  All offsets are 64-bit; out_rec_off and out_hdr_off are 8-byte aligned.
 *      After a call ukm_last_kernel_ms reports the scan between the size side and the write side (its read-backs included),
 *      ukm_last_call_ms the whole call. */
#define UKM_FASTX_FASTQ 1u   /* the text is FASTQ; without it, FASTA */
#define UKM_FASTX_LAST 2u    /* text ends the input: the last record is complete, the last line may lack its LF */
#define UKM_FASTX_STOP_NONE 0     /* everything was consumed */
#define UKM_FASTX_STOP_TAIL 1     /* text[n_consumed, n_bytes) is an incomplete record: call again with more behind it */
#define UKM_FASTX_STOP_GRAMMAR 2  /* text[n_consumed ..] begins something outside the device's grammar: the host parser's */
int ukm_fastx(ukm_ctx *ctx, const uint8_t *text, uint64_t n_bytes, uint32_t flags, uint8_t *out_bases, uint64_t bases_cap,
              uint64_t *out_rec_off /* [rec_cap + 1] */, uint64_t *out_hdr_off /* [rec_cap], may be NULL */, uint64_t rec_cap,
              uint64_t *n_bases, uint64_t *n_rec, uint64_t *n_consumed, int *stop);

/* ---- k-way merge: replaces mergeChunksFile (util-sort.go:227-606).  Streams are expected
 *      to be sorted (chunk files); an unsorted one is tolerated (the call then sorts the
 *      concatenation instead of merging).  mode/final_round as the reference's
 *      unique/repeated/finalRound arguments; equal codes keep stream order. */
int ukm_merge_k(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids,
                const uint64_t *lens, int nstreams, int mode, int final_round,
                uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);

/* ---- 2-way set operation on two SORTED streams — the device hot path that the n-way
 *      entries below are folded from, and what bench.py measures.
 *      Consecutive calls on the SAME two device buffers (same pointers, same sizes: union, then inter, then diff of one
 *      pair) share one internal partition table: the context keeps the most recent one and the next call verifies it
 *      against the buffers as they are now instead of computing it again; a table that no longer fits (the buffers were
 *      rewritten in place) is computed anew.  Results never depend on this cache, only time does.  Host arrays, the n-way
 *      entries and inputs of fewer than ~2.5e6 records in total never use it; statistics "setop_part_hits" /
 *      "setop_part_stale" (ukm_ctx_get_stat).  On plain codes the table carries the pair's match counts too, from which
 *      the later calls know where every tile's output starts (every tile checks its own count; a difference repeats the
 *      pass the usual way): "setop_offs_hits" / "setop_offs_stale". */
int ukm_setop2(ukm_ctx *ctx, int op, const uint64_t *a_keys, const uint32_t *a_taxids,
               uint64_t na, const uint64_t *b_keys, const uint32_t *b_taxids, uint64_t nb,
               uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap,
               uint64_t *n_out);

/* ---- n-way set operations; output is the sorted (code, taxid) stream.
 *      union  : union.go:186-305  (inputs need not be sorted)
 *      inter  : inter.go:188-286  (all inputs sorted)
 *      diff   : diff.go:341-454   (first input sorted; sorted_flags[i]==0 marks unsorted ones,
 *                                  NULL = all sorted)
 *      common : common.go:220-344 (threshold = number of files, common.go:93-105) */
int ukm_union(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids,
              const uint64_t *lens, int nstreams, uint32_t flags, uint64_t *out_keys,
              uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_inter(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids,
              const uint64_t *lens, int nstreams, uint32_t flags, uint64_t *out_keys,
              uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_diff(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids,
             const uint64_t *lens, int nstreams, const uint8_t *sorted_flags, uint32_t flags,
             uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_common(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids,
               const uint64_t *lens, int nstreams, uint32_t threshold, uint32_t flags,
               uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
uint32_t ukm_common_threshold(uint32_t nfiles, double proportion, uint32_t number);

/* ---- per-FILE taxids (round 5).  The reference's documented taxid workflow is ONE taxid per file: `unikmer count -t 511145`
 *      (README.md:170) stores it in the .unik header (count.go:466-468 writer.SetGlobalTaxid) and unik.Reader.ReadCodeWithTaxid
 *      then hands that value out with EVERY record, so union.go:187-201, inter.go:190,211-239, diff.go:404-409 and
 *      common.go:262-266 fold it like a per-record taxid.  The _ft entry points take that value as a scalar instead of an
 *      n-element array of copies:
 *        file_taxids (host array [nstreams], or NULL) / a_file_taxid, b_file_taxid: the taxid of every record of a stream
 *        whose per-record pointer (taxids[i] / a_taxids / b_taxids) is NULL; 0 = the stream has no taxid information (what
 *        a NULL pointer alone means in the entry points above, which are these with file_taxids = NULL).
 *      Results are identical to passing the expanded arrays.  What the device does instead: two streams with one taxid
 *      each run the plain-key kernel and write one of three values (A's, B's, their LCA) per output record; `inter`,
 *      `diff` (also -t: whether file j can take a matched code away is one decision per file) and `common` over all files
 *      are the plain operation and a fill with one value worked out once; the hash-probe `union` / `common` below the number
 *      of files / `merge -d` read no taxid and look no pre-order number up for such a file; the k-way merges get the array
 *      built on the device.  Streams with per-record taxids and streams with one per file may be mixed freely. */
int ukm_setop2_ft(ukm_ctx *ctx, int op, const uint64_t *a_keys, const uint32_t *a_taxids, uint32_t a_file_taxid,
                  uint64_t na, const uint64_t *b_keys, const uint32_t *b_taxids, uint32_t b_file_taxid, uint64_t nb,
                  uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_union_ft(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids, const uint32_t *file_taxids,
                 const uint64_t *lens, int nstreams, uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids,
                 uint64_t out_cap, uint64_t *n_out);
int ukm_inter_ft(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids, const uint32_t *file_taxids,
                 const uint64_t *lens, int nstreams, uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids,
                 uint64_t out_cap, uint64_t *n_out);
int ukm_diff_ft(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids, const uint32_t *file_taxids,
                const uint64_t *lens, int nstreams, const uint8_t *sorted_flags, uint32_t flags, uint64_t *out_keys,
                uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);
int ukm_common_ft(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids, const uint32_t *file_taxids,
                  const uint64_t *lens, int nstreams, uint32_t threshold, uint32_t flags, uint64_t *out_keys,
                  uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);

/* ---- two or three 2-way operations of ONE pair in a single pass: union (union.go:186-208), inter (inter.go:205-278) and
 *      diff (diff.go:379-454) of the same two sorted files -- the reference's README workflow -- read A and B once and write
 *      every requested result from that one merge.
 *      bit (1u << UKM_OP_x) of `ops` asks for operation x; arrays below are indexed by UKM_OP_UNION / _INTER / _DIFF.
 *      For every requested x, out_keys[x], out_taxids[x], n_out[x] and the status are exactly what ukm_setop2_ft with op = x,
 *      the same inputs and flags, and out_cap[x] would give.  Host or device arrays, as there; out_cap[x] == 0 with NULL
 *      arrays is a size query for x; entries of operations that were not requested are neither read nor written
 *      (out_taxids itself may be NULL when no stream carries taxids).  ops == 0 or a bit above UKM_OP_DIFF: UKM_ERR_INVALID.
 *      If any requested output does not fit the call returns UKM_ERR_CAPACITY, EVERY requested n_out[x] holds the size
 *      needed and nothing is written at or behind out_cap[x] of any output.  An unsorted input: UKM_ERR_UNSORTED.
 *      What runs fused: PLAIN codes (both taxid pointers NULL, both file taxids 0), at least two operations, na + nb > 0.
 *      Per-record or per-file taxids, a single operation, and inputs with duplicate codes take one ordinary pass per
 *      operation instead (same results; taxids inside the fused kernel are left to a later version).  The fused pass keeps
 *      a partition table of its own and leaves the cache that consecutive ukm_setop2 calls share untouched.  Statistics
 *      "setop_multi_fused" / "setop_multi_split" (ukm_ctx_get_stat): calls that ended on each route. */
int ukm_setop2_multi(ukm_ctx *ctx, uint32_t ops,
                     const uint64_t *a_keys, const uint32_t *a_taxids, uint32_t a_file_taxid, uint64_t na,
                     const uint64_t *b_keys, const uint32_t *b_taxids, uint32_t b_file_taxid, uint64_t nb,
                     uint32_t flags, uint64_t *const out_keys[3], uint32_t *const out_taxids[3],
                     const uint64_t out_cap[3], uint64_t n_out[3]);
int ukm_merge_k_ft(ukm_ctx *ctx, const uint64_t *const *keys, const uint32_t *const *taxids, const uint32_t *file_taxids,
                   const uint64_t *lens, int nstreams, int mode, int final_round, uint64_t *out_keys,
                   uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out);

/* ---- all-pairs shared code counts of many sets (new: the reference needs N(N-1)/2 runs of `inter | num` for this): what
 *      Jaccard index, containment and Mash distance of 1000 sketches or .unik files are computed from, in one call.
 *      out_counts[i * nstreams + j], i < nrows, j < nstreams: the number of DISTINCT codes that occur in both stream i and
 *      stream j.  out_sizes[j], j < nstreams (may be NULL): the number of distinct codes of stream j (== out_counts[j][j]
 *      where j < nrows).
 *      keys[i]: host or device arrays, mixed freely; they need not be sorted or duplicate-free (a code that repeats inside a
 *      stream counts once), and empty streams give a row and a column of zeros.  1 <= nrows <= nstreams: nrows == nstreams is
 *      the full symmetric matrix, nrows < nstreams the first nrows streams (queries) against all.  1 <= nstreams <= 65536;
 *      flags must be 0; anything else: UKM_ERR_INVALID.  out_counts / out_sizes: host or device; exactly nrows * nstreams
 *      and nstreams items are written.  The result is a pure function of the inputs; counts are 64-bit end to end; running
 *      out of device memory is UKM_ERR_NOMEM.
 *      How: the (code, stream) records of all streams are sorted by code, a distinct code's rank is its column, and the
 *      columns are walked in blocks; per block a bit matrix [stream][column] is set and pair_popc_kernel adds
 *      popcount(row i AND row j) to the counts -- a cost that does not depend on how much the sets overlap.
 *      ukm_last_kernel_ms: the summed time of the pair kernel's launches; ukm_last_call_ms: the whole call.
 *      Statistics (ukm_ctx_get_stat), of the last call: "pair_columns" = distinct codes over all streams, "pair_blocks" =
 *      column blocks walked, "pair_sort_us" / "pair_bits_us" / "pair_kernel_us" = device time in microseconds of the sort
 *      and ranking step, of zeroing and setting the bits, and of the pair kernel.  Option "pair_block_cols" (developer and
 *      test knob): columns per block, rounded up to whole K tiles of 2048; unset: the widest block whose bit matrix stays
 *      within 1 GiB.  Results never depend on it. */
int ukm_pair_counts(ukm_ctx *ctx, const uint64_t *const *keys, const uint64_t *lens, int nstreams, int nrows,
                    uint32_t flags, uint64_t *out_counts, uint64_t *out_sizes);

/* ---- which records belong to a set (new: the reference would run `count` on every record and `inter | num` the result, one
 *      process per record): per record the number of windows, the number of windows whose value is in a sorted code set, and
 *      the LCA of the taxids of those hits.  Reads against a host or contaminant set, contigs against a taxon-annotated
 *      database, a marker set against a sample.
 *      bases / rec_off as for ukm_encode_kmers (host or device, rec_off[0] == 0); canonical / circular / hashed select the
 *      windows exactly as ukm_encode_kmers (hashed = 0) and ukm_nthash with max_hash = 0 (hashed = 1) produce them.
 *      set_keys[n_set]: ascending, duplicates tolerated (UKM_ERR_UNSORTED otherwise, as ukm_map); set_taxids: NULL or n_set
 *      values.  All pointers may be host or device pointers.
 *      Outputs, exactly n_rec entries each, each may be NULL:
 *        out_win[r] = the number of windows of record r (0 for a record shorter than k);
 *        out_hit[r] = the number of those windows whose value is in set_keys; every window counts, repeated codes included;
 *        out_lca[r] = 0 when out_hit[r] == 0, else the LEFT FOLD of ukm_lca's pairwise contract over the taxids of the
 *          record's hit windows in window order, a hit's taxid being set_taxids[i] with i the FIRST index where
 *          set_keys[i] == code.  That fold equals a closed form, which is what is computed (the argument: DESIGN.md 4.24): the
 *          common value when all hit taxids are the same number (also an id the taxonomy does not know, also 0, also a
 *          merged id, which stays unmapped); otherwise 0 when any hit taxid is 0 or absent after merged ids are remapped;
 *          otherwise the LCA of the set (0 when it spans different trees).
 *      Errors: UKM_ERR_K, UKM_ERR_ILLEGAL_BASE as the window calls give them; UKM_ERR_INVALID for a NULL ctx, for out_lca
 *      without set_taxids, and for 2^32 or more windows, records or set codes in one call (split the records over several
 *      calls); UKM_ERR_NO_TAXONOMY when out_lca and set_taxids are given and no taxonomy is loaded.  After an error nothing is
 *      promised about the outputs.  n_rec == 0: UKM_OK, nothing is done.  n_set == 0: every out_hit / out_lca entry is 0,
 *      out_win is filled.
 *      How: the windows of all records (ukm_encode.hip) are joined against the set through its prefix
 *      directory, and one workgroup per tile of consecutive windows folds hits, min / max raw taxid and min / max pre-order
 *      number into per-record state: records inside a tile by plain stores, the two that cross its edges by atomics.  Context
 *      option "map_sorted" as for ukm_map: 0 the windows look their codes up in genome order (nothing per window is written),
 *      1 all (code, window) pairs are sorted first and one 32-bit word per window comes back; default: by the size of the set
 *      (a threshold inherited from ukm_map).  ukm_last_kernel_ms: the lookup and reduction kernels. */
int ukm_screen(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, int k, int canonical, int circular,
               int hashed, const uint64_t *set_keys, const uint32_t *set_taxids, uint64_t n_set, uint32_t *out_win,
               uint32_t *out_hit, uint32_t *out_lca);

/* ---- multi-GPU helper: split points of a sorted stream for prefix sharding (SURVEY.md
 *      §8(e)): cuts[g] = lower_bound(keys, splitters[g]) for g in [0, n_split). */
int ukm_partition_points(ukm_ctx *ctx, const uint64_t *keys, uint64_t n,
                         const uint64_t *splitters, int n_split, uint64_t *cuts);

/* ---- multi-GPU exchange over RCCL / xGMI (new): one process and one ukm_ctx per GPU.
 *      The reference is single-process; this is the step that lets a host shard the code space by high-bits prefix:
 *        ukm_prefix_splitters -> ukm_partition_points (cuts of every local sorted file) -> ukm_shard_exchange (slice g
 *        of every rank travels to rank g) -> ukm_union / ukm_merge_k of the received slices -> the 1-GPU operation on
 *        the rank's range; the ranks' results concatenated in rank order are the global sorted result.
 *      ukm_comm_get_unique_id: 128 opaque bytes (ncclUniqueId) made by ONE rank and handed to the others by the host
 *      (file, socket, MPI ...).  ukm_comm_init is collective.  RCCL is loaded on first use (dlopen): a single-GPU host
 *      needs no RCCL at all.
 *      ukm_shard_exchange: send_counts[nranks] (host) = number of consecutive records of keys/taxids for each rank in
 *      rank order (their sum is the stream length); recv_counts[nranks] (host, out) = records received from each rank;
 *      the received slices are stored back to back in source-rank order (each is sorted; together they are this rank's
 *      range of the logical file).  keys / taxids / out_* may be host or device pointers. */
#define UKM_COMM_ID_BYTES 128
int ukm_comm_get_unique_id(void *id);
int ukm_comm_init(ukm_ctx *ctx, int nranks, int rank, const void *id);
int ukm_comm_destroy(ukm_ctx *ctx);
int ukm_comm_info(ukm_ctx *ctx, int *nranks, int *rank);
int ukm_prefix_splitters(int key_bits, int nranks, uint64_t *splitters);
int ukm_shard_exchange(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, const uint64_t *send_counts,
                       uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *recv_counts, uint64_t *n_out);
/*      Capacity is decided COLLECTIVELY: the slice sizes travel together with every rank's out_cap, and either all
 *      ranks exchange or all ranks return UKM_ERR_CAPACITY (n_out = what this rank would have received), so a short
 *      buffer on one rank can never leave its peers blocked in RCCL.  ukm_shard_plan is that decision as a pure host
 *      function (all = [source rank][nranks slice sizes | out_cap of the source rank], the gathered matrix; bit 63 of
 *      the capacity word = UKM_SHARD_HAS_TAXIDS, "this rank passed taxids": ranks that disagree all return UKM_ERR_INVALID
 *      before anything is posted -- a mixed call would leave taxid transfers unmatched).
 *      Hosts that move many files use the two-step form: ukm_shard_counts (send_counts[nfiles][nranks] ->
 *      recv_counts[nfiles][nranks], ONE all-gather and host round trip for all files; size the receive buffers
 *      from it), then ukm_shard_exchange_known per file, which has no gather and no host round trip in front of the
 *      transfers (own slice: device-to-device copy; peers: one ncclSend / ncclRecv group on the context's stream; like
 *      every entry point the call returns when its stream work is done).  It takes no collective decision: a rank whose
 *      buffer is too small, or whose own entries of send_counts / recv_counts disagree, still takes part (what arrives is
 *      dropped in a scratch buffer of the largest slice) and returns UKM_ERR_CAPACITY / UKM_ERR_INVALID afterwards.  A
 *      device failure in front of the transfers (no memory for staging) leaves the peers blocked in RCCL: destroy the
 *      communicator, as after any lost rank.  Files WITH taxids: pass ukm_shard_counts_tax the flags has_taxids[nfiles]
 *      (1: this rank will hand ukm_shard_exchange_known a taxid array for file f); the flags ride in the same gather and
 *      ranks that disagree about a file all get UKM_ERR_INVALID here, before any transfer is posted
 *      (ukm_shard_counts_plan: that decision as a pure host function over the gathered words, [rank][nfiles * nranks slice
 *      sizes | nfiles flags, 2 = not declared]). */
#define UKM_SHARD_HAS_TAXIDS (1ull << 63)
#define UKM_SHARD_RANK_FAILED (~0ull) /* ukm_shard_splitters: a rank's record-count word when its preparation failed */
int ukm_shard_plan(int nranks, int rank, const uint64_t *all, uint64_t *recv_counts, uint64_t *n_out);
/*      Sampled splitters (k-mer codes are not uniform in their top bits -- README.md:177-180, sorted
 *      k-mers start AAAAAAAAA... -- so equal-width ranges leave the ranks unevenly loaded): ukm_shard_splitters is
 *      collective; every rank passes the sorted files it holds and gets the same nranks + 1 boundaries, cut so that the
 *      ranks receive about the same number of records (1024 regular samples per rank, one all-gather).  Use them in
 *      place of ukm_prefix_splitters; any non-decreasing boundaries give the same concatenated result.  A rank that
 *      fails locally (bad argument, no memory for staging) still takes part in the gather -- with UKM_SHARD_RANK_FAILED as
 *      its record count -- and returns its error afterwards; EVERY other rank then returns UKM_ERR_PEER, so all hosts
 *      abort the exchange together (nobody goes on to ukm_shard_counts with a rank missing); only a rank that cannot even
 *      allocate the 8 KB gather buffers hangs its peers (destroy the communicator, as after any lost rank).  Host arrays
 *      are sampled where they lie.
 *      ukm_shard_splitters_plan is the decision as a pure host function over the gathered words
 *      ([rank][1 + per_rank] = record count, samples). */
int ukm_shard_splitters(ukm_ctx *ctx, const uint64_t *const *keys, const uint64_t *lens, int nfiles, int key_bits,
                        uint64_t *splitters);
int ukm_shard_splitters_plan(int nranks, int per_rank, const uint64_t *all, int key_bits, uint64_t *splitters);
int ukm_shard_counts(ukm_ctx *ctx, const uint64_t *send_counts, int nfiles, uint64_t *recv_counts);
int ukm_shard_counts_tax(ukm_ctx *ctx, const uint64_t *send_counts, int nfiles, const uint8_t *has_taxids, uint64_t *recv_counts);
int ukm_shard_counts_plan(int nranks, int rank, int nfiles, const uint64_t *all, uint64_t *recv_counts);
int ukm_shard_exchange_known(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, const uint64_t *send_counts,
                             const uint64_t *recv_counts, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap,
                             uint64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
