"""ctypes binding of libunikmer_hip.so (C ABI: include/unikmer_hip.h).

There is NO CPU fallback: if the HIP library is missing, cannot be loaded, or no GPU is
present, calls raise.  Arrays may be numpy arrays (host) or torch tensors (host or device);
device tensors are passed by data_ptr and never copied.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# UKM_LIB_PATH: developer override to load an experimental build of the same HIP library
SO_PATH = os.environ.get("UKM_LIB_PATH") or os.path.join(_HERE, "libunikmer_hip.so")

OK = 0
ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_ILLEGAL_BASE = -1, -2, -3, -4
ERR_UNSORTED, ERR_NO_TAXONOMY, ERR_CAPACITY, ERR_K, ERR_PEER = -5, -6, -7, -8, -9
ERR_FORMAT = -10   # a .unik body ends inside a record; a line of k-mer text outside the grammar of ukm_dump
UNIK_COMPACT, UNIK_SORTED, UNIK_INCLUDE_TAXID = 1, 4, 8   # header flag bits the .unik codec looks at (unik.hpp)
# ukm_view formats and ukm_dump flags (include/unikmer_hip.h: UKM_VIEW_*, UKM_DUMP_*)
VIEW_KMER, VIEW_KMER_CODE, VIEW_CODE, VIEW_KMER_TAXID, VIEW_TAXID, VIEW_FASTA, VIEW_FASTQ = range(7)
VIEW_WITH_TAXID = 16
DUMP_TAXID, DUMP_DECIMAL, DUMP_CANONICAL, DUMP_CANONICAL_ONLY = 1, 2, 4, 8
# ukm_fastx flags and stop reasons (include/unikmer_hip.h: UKM_FASTX_*)
FASTX_FASTQ, FASTX_LAST = 1, 2
FASTX_STOP_NONE, FASTX_STOP_TAIL, FASTX_STOP_GRAMMAR = 0, 1, 2
PLAIN, UNIQUE, REPEATED, REPEATED_CHUNK, SINGLETON = 0, 1, 2, 3, 4
OP_UNION, OP_INTER, OP_DIFF = 0, 1, 2
F_MIX_TAXID, F_CMP_TAXID = 2, 4
F_INVERT, F_QUERY_TAXID = 8, 16   # grep -v / filter -v; grep -t
F_DEVICE_STREAMS = 256   # every stream pointer of an n-way call is a device pointer (no per-pointer driver query)
# Context.last_route(): which internal route answered the last n-way call (include/unikmer_hip.h: UKM_ROUTE_*)
ROUTE_NONE, ROUTE_TREE, ROUTE_KWAY, ROUTE_PUNION, ROUTE_SRMERGE, ROUTE_SRCOMMON, ROUTE_PCOMMON, ROUTE_PLACE = range(8)

# every symbol include/unikmer_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "ukm_last_error", "ukm_version", "ukm_device_count", "ukm_ctx_create", "ukm_ctx_destroy",
    "ukm_ctx_set_stream", "ukm_ctx_sync", "ukm_ctx_reserve", "ukm_ctx_trim", "ukm_dev_alloc", "ukm_dev_free",
    "ukm_copy", "ukm_host_alloc", "ukm_host_free", "ukm_copy_async", "ukm_copy_fence", "ukm_copy_sync", "ukm_last_kernel_ms", "ukm_last_call_ms", "ukm_last_route", "ukm_taxonomy_load", "ukm_taxonomy_max_taxid", "ukm_lca",
    "ukm_encode_kmers", "ukm_nthash", "ukm_minimizer", "ukm_max_hash", "ukm_sort_u64", "ukm_sort_pairs",
    "ukm_unique", "ukm_merge_k", "ukm_setop2", "ukm_union", "ukm_inter", "ukm_diff",
    "ukm_common", "ukm_common_threshold", "ukm_partition_points",
    "ukm_comm_get_unique_id", "ukm_comm_init", "ukm_comm_destroy", "ukm_comm_info", "ukm_prefix_splitters",
    "ukm_shard_exchange", "ukm_shard_plan", "ukm_shard_counts", "ukm_shard_exchange_known",
    "ukm_shard_splitters", "ukm_shard_splitters_plan", "ukm_shard_counts_tax", "ukm_shard_counts_plan", "ukm_count",
    "ukm_ctx_set_option", "ukm_ctx_unset_option", "ukm_ctx_get_option", "ukm_ctx_get_stat",
    "ukm_setop2_ft", "ukm_union_ft", "ukm_inter_ft", "ukm_diff_ft", "ukm_common_ft", "ukm_merge_k_ft",
    "ukm_locate", "ukm_map", "ukm_map_gapped", "ukm_grep", "ukm_filter", "ukm_sample",
    "ukm_taxonomy_set_ranks", "ukm_rank_filter_plan", "ukm_rank_pass", "ukm_rfilter", "ukm_tsplit",
    "ukm_unik_decode", "ukm_unik_encode", "ukm_unik_encode_bound",
    "ukm_view", "ukm_view_bound", "ukm_dump",
    "ukm_deflate", "ukm_deflate_bound", "ukm_crc32_combine",
    "ukm_inflate", "ukm_inflate_bound",
    "ukm_fastx",
    "ukm_setop2_multi",
    "ukm_pair_counts",
    "ukm_screen",
]


class RankFilter(C.Structure):
    """ukm_rank_filter (include/unikmer_hip.h): a rank filter stated in rank ids and orders.  RankFilter.make builds one
    from plain Python values."""
    _fields_ = [("order", C.c_int32 * 256), ("no_rank", C.c_uint8 * 256), ("black", C.c_uint8 * 256),
                ("lower", C.c_int32), ("higher", C.c_int32), ("equal", C.c_int32 * 32), ("n_equal", C.c_int32),
                ("discard_norank", C.c_uint8), ("save_norank", C.c_uint8), ("discard_root", C.c_uint8),
                ("root_taxid", C.c_uint32)]

    @classmethod
    def make(cls, order=None, no_rank=(), black=(), lower=0, higher=0, equal=(), discard_norank=False, save_norank=False,
             discard_root=False, root_taxid=1):
        """order: {rank id: order > 0}; no_rank / black: rank ids; lower / higher / equal: ORDERS (0 = not given)"""
        f = cls()
        for r, o in (order or {}).items():
            f.order[int(r)] = int(o)
        for r in no_rank:
            f.no_rank[int(r)] = 1
        for r in black:
            f.black[int(r)] = 1
        f.lower, f.higher = int(lower), int(higher)
        equal = list(equal)
        for i, o in enumerate(equal[:32]):
            f.equal[i] = int(o)
        f.n_equal = len(equal)          # (more than 32: the library refuses it)
        f.discard_norank, f.save_norank, f.discard_root = int(bool(discard_norank)), int(bool(save_norank)), int(bool(discard_root))
        f.root_taxid = int(root_taxid)
        return f



class UkmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libunikmer_hip error %d: %s" % (code, msg))
        self.code = code


class IllegalBaseError(UkmError):
    pass


class UnsortedError(UkmError):
    pass


class FormatError(UkmError):
    """a .unik body ends inside a record, or a line of k-mer text is outside the grammar of ukm_dump (UKM_ERR_FORMAT);
    bad_off: the byte offset at which that line starts (ukm_dump only)"""
    bad_off = None


class CapacityError(UkmError):
    """out_cap was too small; `needed` is the size the library reported in *n_out (None where a call reports none)"""

    def __init__(self, code, msg, needed=None):
        super().__init__(code, msg)
        self.needed = needed


_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7).  If ours were loaded from /opt/rocm first, a later `import torch` would
    bring up a second runtime that sees no GPU.  Loading torch's copy first (without importing
    torch) makes the dynamic loader bind libunikmer_hip.so to it by SONAME."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """dlopen the HIP library; raises if it has not been built (python -m unikmer_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError("libunikmer_hip.so is not built (%s); run `python -m unikmer_amd.build`. "
                          "There is no CPU fallback." % SO_PATH)
    _preload_hip_runtime()
    L = C.CDLL(SO_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    pu64 = C.POINTER(C.c_uint64)
    pvp = C.POINTER(C.c_void_p)
    L.ukm_last_error.restype = C.c_char_p
    L.ukm_version.restype = i32
    L.ukm_device_count.argtypes = [C.POINTER(i32)]
    L.ukm_ctx_create.argtypes = [i32, pvp]
    L.ukm_ctx_destroy.argtypes = [vp]
    L.ukm_ctx_set_stream.argtypes = [vp, vp]
    L.ukm_ctx_sync.argtypes = [vp]
    L.ukm_ctx_reserve.argtypes = [vp, u64]
    L.ukm_ctx_trim.argtypes = [vp]
    L.ukm_dev_alloc.argtypes = [vp, u64, pvp]
    L.ukm_dev_free.argtypes = [vp, vp]
    L.ukm_copy.argtypes = [vp, vp, vp, u64]
    L.ukm_host_alloc.argtypes = [vp, u64, pvp]
    L.ukm_host_free.argtypes = [vp, vp]
    L.ukm_copy_async.argtypes = [vp, vp, vp, u64]
    L.ukm_copy_fence.argtypes = [vp]
    L.ukm_copy_sync.argtypes = [vp]
    L.ukm_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ukm_last_call_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ukm_last_route.argtypes = [vp]
    L.ukm_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_longlong]
    L.ukm_ctx_unset_option.argtypes = [vp, C.c_char_p]
    L.ukm_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(i32)]
    L.ukm_ctx_get_stat.argtypes = [vp, C.c_char_p, C.POINTER(C.c_ulonglong)]
    L.ukm_taxonomy_load.argtypes = [vp, vp, vp, u64, vp, vp, u64]
    L.ukm_taxonomy_max_taxid.argtypes = [vp, C.POINTER(u32)]
    L.ukm_lca.argtypes = [vp, vp, vp, u64, vp]
    L.ukm_encode_kmers.argtypes = [vp, vp, vp, u64, i32, i32, i32, vp, u64, pu64]
    L.ukm_nthash.argtypes = [vp, vp, vp, u64, i32, i32, i32, u64, vp, u64, pu64]
    L.ukm_count.argtypes = [vp, vp, vp, u64, i32, i32, i32, i32, u64, i32, vp, u64, pu64]
    L.ukm_locate.argtypes = [vp, vp, vp, u64, i32, i32, i32, vp, u64, vp, vp, vp, u64, pu64]
    L.ukm_map.argtypes = [vp, vp, vp, u64, vp, u64, i32, i32, vp, u64, i32, u64, vp, vp, vp, u64, pu64]
    L.ukm_map_gapped.argtypes = [vp, vp, vp, u64, vp, u64, i32, i32, i32, vp, u64, i32, u64, u64, u64, vp, vp, vp, u64, pu64]
    L.ukm_screen.argtypes = [vp, vp, vp, u64, i32, i32, i32, i32, vp, vp, u64, vp, vp, vp]
    L.ukm_grep.argtypes = [vp, vp, vp, u32, u64, i32, vp, vp, u64, u32, vp, vp, u64, pu64]
    L.ukm_filter.argtypes = [vp, vp, vp, u64, i32, i32, i32, i32, i32, u32, vp, vp, u64, pu64]
    L.ukm_sample.argtypes = [vp, vp, vp, u64, u64, u64, vp, vp, u64, pu64]
    L.ukm_taxonomy_set_ranks.argtypes = [vp, vp, vp, u64]
    L.ukm_rank_filter_plan.argtypes = [vp, vp, vp]
    L.ukm_rank_pass.argtypes = [vp, vp, vp, u64, vp]
    L.ukm_rfilter.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp, u64, pu64]
    L.ukm_tsplit.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, u64, pu64]
    L.ukm_unik_decode.argtypes = [vp, vp, u64, i32, u32, i32, vp, vp, u64, pu64]
    L.ukm_unik_encode.argtypes = [vp, vp, vp, u64, i32, u32, i32, vp, u64, pu64]
    L.ukm_unik_encode_bound.argtypes = [u64, i32, u32, i32]
    L.ukm_unik_encode_bound.restype = u64
    L.ukm_view.argtypes = [vp, vp, vp, u32, u64, i32, i32, u32, vp, u64, pu64]
    L.ukm_view_bound.argtypes = [u64, i32, i32, u32]
    L.ukm_view_bound.restype = u64
    L.ukm_dump.argtypes = [vp, vp, u64, i32, u32, vp, vp, u64, pu64, pu64]
    L.ukm_deflate.argtypes = [vp, vp, u64, u32, vp, u64, pu64, C.POINTER(u32)]
    L.ukm_deflate_bound.argtypes = [u64, u32]
    L.ukm_deflate_bound.restype = u64
    L.ukm_inflate.argtypes = [vp, vp, u64, u32, vp, u64, pu64, pu64, C.POINTER(u32)]
    L.ukm_inflate_bound.argtypes = [u64]
    L.ukm_inflate_bound.restype = u64
    L.ukm_fastx.argtypes = [vp, vp, u64, u32, vp, u64, vp, vp, u64, pu64, pu64, pu64, C.POINTER(i32)]
    L.ukm_crc32_combine.argtypes = [u32, u32, u64]
    L.ukm_crc32_combine.restype = u32
    L.ukm_minimizer.argtypes = [vp, vp, vp, u64, i32, i32, i32, u64, vp, vp, u64, pu64]
    L.ukm_max_hash.argtypes = [u64]
    L.ukm_max_hash.restype = u64
    L.ukm_sort_u64.argtypes = [vp, vp, u64, i32]
    L.ukm_sort_pairs.argtypes = [vp, vp, vp, u64, i32]
    L.ukm_unique.argtypes = [vp, vp, vp, u64, i32, vp, vp, u64, pu64]
    L.ukm_merge_k.argtypes = [vp, pvp, pvp, pu64, i32, i32, i32, vp, vp, u64, pu64]
    L.ukm_setop2.argtypes = [vp, i32, vp, vp, u64, vp, vp, u64, u32, vp, vp, u64, pu64]
    for f in (L.ukm_union, L.ukm_inter):
        f.argtypes = [vp, pvp, pvp, pu64, i32, u32, vp, vp, u64, pu64]
    L.ukm_diff.argtypes = [vp, pvp, pvp, pu64, i32, vp, u32, vp, vp, u64, pu64]
    L.ukm_common.argtypes = [vp, pvp, pvp, pu64, i32, u32, u32, vp, vp, u64, pu64]
    # per-FILE taxids (one value per stream: the .unik header's global taxid)
    L.ukm_merge_k_ft.argtypes = [vp, pvp, pvp, vp, pu64, i32, i32, i32, vp, vp, u64, pu64]
    L.ukm_setop2_ft.argtypes = [vp, i32, vp, vp, u32, u64, vp, vp, u32, u64, u32, vp, vp, u64, pu64]
    L.ukm_setop2_multi.argtypes = [vp, u32, vp, vp, u32, u64, vp, vp, u32, u64, u32, pvp, pvp, pu64, pu64]
    L.ukm_pair_counts.argtypes = [vp, pvp, pu64, i32, i32, u32, vp, vp]
    for f in (L.ukm_union_ft, L.ukm_inter_ft):
        f.argtypes = [vp, pvp, pvp, vp, pu64, i32, u32, vp, vp, u64, pu64]
    L.ukm_diff_ft.argtypes = [vp, pvp, pvp, vp, pu64, i32, vp, u32, vp, vp, u64, pu64]
    L.ukm_common_ft.argtypes = [vp, pvp, pvp, vp, pu64, i32, u32, u32, vp, vp, u64, pu64]
    L.ukm_common_threshold.argtypes = [u32, C.c_double, u32]
    L.ukm_common_threshold.restype = u32
    L.ukm_partition_points.argtypes = [vp, vp, u64, vp, i32, vp]
    L.ukm_comm_get_unique_id.argtypes = [vp]
    L.ukm_comm_init.argtypes = [vp, i32, i32, vp]
    L.ukm_comm_destroy.argtypes = [vp]
    L.ukm_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.ukm_prefix_splitters.argtypes = [i32, i32, vp]
    L.ukm_shard_exchange.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, pu64]
    L.ukm_shard_plan.argtypes = [i32, i32, vp, vp, pu64]
    L.ukm_shard_counts.argtypes = [vp, vp, i32, vp]
    L.ukm_shard_counts_tax.argtypes = [vp, vp, i32, vp, vp]
    L.ukm_shard_counts_plan.argtypes = [i32, i32, i32, vp, vp]
    L.ukm_shard_exchange_known.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, pu64]
    L.ukm_shard_splitters.argtypes = [vp, pvp, pu64, i32, i32, vp]
    L.ukm_shard_splitters_plan.argtypes = [i32, i32, vp, i32, vp]
    _lib = L
    return L


class StreamTable:
    """see Context.stream_table"""

    def __init__(self, args, ref):
        self.args = args
        self.ref = ref


def _check(rc, needed=None):
    """needed: the call's n_out (UKM_ERR_CAPACITY leaves the required size there: the two-call idiom)"""
    if rc == OK:
        return
    msg = load().ukm_last_error().decode(errors="replace")
    if rc == ERR_CAPACITY:
        raise CapacityError(rc, msg, None if needed is None else int(needed))
    cls = {ERR_ILLEGAL_BASE: IllegalBaseError, ERR_UNSORTED: UnsortedError, ERR_FORMAT: FormatError}.get(rc, UkmError)
    raise cls(rc, msg)


def _sized(call, outs, alloc):
    """The size-query form of the two-call idiom: call(outs) -> (rc, n_out) runs an entry point on the caller's outputs; outs None:
    call(None) asks first (NULL outputs, capacity 0: UKM_ERR_CAPACITY means n_out is the size), alloc(n_out) makes them.  Returns (outs, n_out)."""
    if outs is None:
        rc, n = call(None)
        if rc != ERR_CAPACITY:
            _check(rc)
        outs = alloc(int(n))
    rc, n = call(outs)
    _check(rc, n)
    return outs, int(n)


def _sized_records(call, ref, tax, out, out_taxids, empty):
    """_sized for an entry point that leaves records: call(po, pot, cap) -> (rc, n_out).  The outputs are a pair: keys (`out`) and, when
    `tax` (the records carry taxids), taxids beside them, each made where `ref` lives when not given.  empty: no input, capacity 0."""
    def pair(keys):
        return keys, ((_empty_like_kind(ref, _ptr(keys, np.uint64)[1], np.uint32) if out_taxids is None else out_taxids) if tax else None)

    def run(o):
        po, cap, _ = _ptr(o and o[0], np.uint64)
        pot, ncap, _ = _ptr(o and o[1], np.uint32)
        return call(po, pot, 0 if empty else min(cap, ncap) if tax else cap)
    (keys, taxids), n = _sized(run, None if out is None else pair(out), lambda need: pair(_empty_like_kind(ref, need, np.uint64)))
    return keys[:n], (taxids[:n] if tax else None)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _is_file_taxid(t):
    """a stream's taxids given as ONE number: the file's global taxid (every record carries it)"""
    return isinstance(t, (int, np.integer))


_NP2TORCH = {np.dtype(np.uint64): "int64", np.dtype(np.uint32): "int32", np.dtype(np.uint8): "uint8"}


def _ptr(x, dtype):
    """(pointer, length, keepalive) of a numpy array / torch tensor viewed as `dtype` items."""
    if x is None:
        return None, 0, None
    if _is_torch(x):
        assert x.is_contiguous(), "tensors passed to libunikmer_hip must be contiguous"
        assert x.element_size() == np.dtype(dtype).itemsize, "tensor item size mismatch"
        return x.data_ptr() if x.numel() else None, x.numel(), x
    a = np.ascontiguousarray(x, dtype=dtype)
    return (a.ctypes.data if a.size else None), a.size, a


def _empty_like_kind(ref, n, dtype):
    """allocate an output of n items where `ref` lives (device tensor -> device tensor)."""
    if _is_torch(ref):
        import torch
        return torch.empty(max(n, 1), dtype=getattr(torch, _NP2TORCH[np.dtype(dtype)]), device=ref.device)
    return np.empty(max(n, 1), dtype=dtype)


def unik_encode_bound(n, k, flags, taxid_bytes=0):
    """bytes a .unik body of n records takes at most (exact for the unsorted layouts); pure host code"""
    return int(load().ukm_unik_encode_bound(int(n), int(k), int(flags), int(taxid_bytes)))


def view_bound(n, k, hashed=False, fmt=VIEW_KMER):
    """bytes the text of n records takes at most (exact for VIEW_KMER of codes that are not hashed); pure host code"""
    return int(load().ukm_view_bound(int(n), int(k), int(bool(hashed)), int(fmt)))


DEFLATE_FINAL, DEFLATE_GZIP = 1, 2   # include/unikmer_hip.h: UKM_DEFLATE_*


def deflate_bound(n_bytes, final=False, gzip=False):
    """bytes Context.deflate writes at most for n_bytes of input; pure host code"""
    return int(load().ukm_deflate_bound(int(n_bytes), (DEFLATE_FINAL if final else 0) | (DEFLATE_GZIP if gzip else 0)))


def inflate_bound(n_bytes):
    """8 * n_bytes: what n_bytes of deflate blocks inflate to at most under Context.inflate (a literal costs at least one
    bit) -- a worst case that nobody should allocate: ask for the size, or take it from the gzip trailer; pure host code"""
    return int(load().ukm_inflate_bound(int(n_bytes)))


def crc32_combine(crc_a, crc_b, len_b):
    """the CRC-32 of A followed by B from zlib.crc32(A), zlib.crc32(B) and len(B); pure host code"""
    return int(load().ukm_crc32_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


class Context:
    """One ukm_ctx: a HIP stream + device workspace.  Not thread-safe (one per thread)."""

    def __init__(self, device=0, stream=None):
        """stream: a hipStream_t handle to borrow (0 = HIP's default stream, e.g.
        torch.cuda.current_stream().cuda_stream); None = the ctx creates its own stream, in
        which case the caller must synchronise its own producers before calling."""
        L = load()
        n = C.c_int(0)
        L.ukm_device_count(C.byref(n))
        if n.value == 0:
            raise RuntimeError("libunikmer_hip: no HIP device visible; this path has no CPU fallback")
        h = C.c_void_p()
        _check(L.ukm_ctx_create(device, C.byref(h)))
        self.h = h
        self.L = L
        if stream is not None:
            _check(L.ukm_ctx_set_stream(self.h, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "h", None):
            self.L.ukm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing ----
    def set_stream(self, stream):
        _check(self.L.ukm_ctx_set_stream(self.h, C.c_void_p(stream)))

    def sync(self):
        _check(self.L.ukm_ctx_sync(self.h))

    def reserve(self, nbytes):
        _check(self.L.ukm_ctx_reserve(self.h, nbytes))

    def trim(self):
        """give the device workspace back (it is kept at the size the largest call needed)"""
        _check(self.L.ukm_ctx_trim(self.h))

    # device / pinned host memory and copies (include/unikmer_hip.h).  Pointers are plain integers; `dst` / `src` of the
    # copies are such integers (or anything C.c_void_p takes), `nbytes` bytes each.
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        _check(self.L.ukm_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        _check(self.L.ukm_dev_free(self.h, C.c_void_p(ptr)))

    def copy(self, dst, src, nbytes):
        """synchronous copy on the context's stream, any direction"""
        _check(self.L.ukm_copy(self.h, C.c_void_p(dst), C.c_void_p(src), nbytes))

    def host_alloc(self, nbytes):
        """pinned host memory: what copy_async needs to overlap with compute"""
        p = C.c_void_p()
        _check(self.L.ukm_host_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def host_free(self, ptr):
        _check(self.L.ukm_host_free(self.h, C.c_void_p(ptr)))

    def copy_async(self, dst, src, nbytes):
        """copy on the context's transfer stream, ordered behind the compute calls issued so far"""
        _check(self.L.ukm_copy_async(self.h, C.c_void_p(dst), C.c_void_p(src), nbytes))

    def copy_fence(self):
        """compute calls issued after the fence start after the transfers issued before it"""
        _check(self.L.ukm_copy_fence(self.h))

    def copy_sync(self):
        """wait for the transfers issued so far"""
        _check(self.L.ukm_copy_sync(self.h))

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(self.L.ukm_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def last_route(self):
        """which internal route answered the last n-way call (include/unikmer_hip.h: ukm_last_route)"""
        return int(self.L.ukm_last_route(self.h))

    def set_option(self, key, value):
        """route policy of this context (include/unikmer_hip.h: ukm_ctx_set_option); value None removes the override"""
        if value is None:
            _check(self.L.ukm_ctx_unset_option(self.h, key.encode()))
        else:
            _check(self.L.ukm_ctx_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v, s = C.c_longlong(), C.c_int()
        _check(self.L.ukm_ctx_get_option(self.h, key.encode(), C.byref(v), C.byref(s)))
        return int(v.value) if s.value else None

    def stat(self, key):
        v = C.c_ulonglong()
        _check(self.L.ukm_ctx_get_stat(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def last_call_ms(self):
        ms = C.c_float()
        _check(self.L.ukm_last_call_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- taxonomy ----
    def taxonomy_load(self, child, parent, merged_old=None, merged_new=None):
        pc, n, k1 = _ptr(child, np.uint32)
        pp, n2, k2 = _ptr(parent, np.uint32)
        assert n == n2
        po, m, k3 = _ptr(merged_old, np.uint32)
        pn, m2, k4 = _ptr(merged_new, np.uint32)
        assert m == m2
        _check(self.L.ukm_taxonomy_load(self.h, pc, pp, n, po, pn, m))

    def max_taxid(self):
        v = C.c_uint32()
        _check(self.L.ukm_taxonomy_max_taxid(self.h, C.byref(v)))
        return v.value

    def lca(self, a, b, out=None):
        pa, n, k1 = _ptr(a, np.uint32)
        pb, n2, k2 = _ptr(b, np.uint32)
        assert n == n2
        if out is None:
            out = _empty_like_kind(a, n, np.uint32)
        po, no, _ = _ptr(out, np.uint32)
        assert no >= n
        _check(self.L.ukm_lca(self.h, pa, pb, n, po))
        return out[:n]

    def taxonomy_set_ranks(self, child, rank_id):
        """rank_id[i] in 1..255 = the rank of child[i] (the caller numbers the rank names), 0 = no known rank"""
        pc, n, k1 = _ptr(child, np.uint32)
        pr, n2, k2 = _ptr(rank_id, np.uint8)
        assert n == n2
        _check(self.L.ukm_taxonomy_set_ranks(self.h, pc, pr, n))

    @staticmethod
    def rank_filter_plan(f):
        """the decision of a RankFilter per rank id, as the pure host function the device pass uses: (self_action, walk_action),
        256 bytes each (include/unikmer_hip.h: ukm_rank_filter_plan)"""
        sa, wa = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
        _check(load().ukm_rank_filter_plan(C.addressof(f), sa.ctypes.data, wa.ctypes.data))
        return sa, wa

    def rank_pass(self, f, taxids, out=None):
        """1 where a record with that taxid passes the RankFilter, else 0 (rfilter.go:438-520)"""
        pt, n, k1 = _ptr(taxids, np.uint32)
        if out is None:
            out = _empty_like_kind(taxids, n, np.uint8)
        po, no, _ = _ptr(out, np.uint8)
        assert no >= n
        _check(self.L.ukm_rank_pass(self.h, C.addressof(f), pt, n, po))
        return out[:n]

    # ---- encode / hash ----
    def _windows(self, fn, bases, rec_off, k, canonical, circular, max_hash, out):
        pb, nb, k1 = _ptr(bases, np.uint8)
        poff, noff, k2 = _ptr(rec_off, np.uint64)
        n_rec = noff - 1
        if out is None:
            if _is_torch(rec_off):
                lens = (rec_off[1:] - rec_off[:-1])
                cap = int(lens.sum().item()) if circular else int(lens.clamp(min=k - 1).sub(k - 1).sum().item())
            else:
                lens = np.diff(np.asarray(rec_off).astype(np.int64))
                cap = int(lens.sum()) if circular else int(np.maximum(lens - (k - 1), 0).sum())
            out = _empty_like_kind(bases, cap, np.uint64)
        po, cap, _ = _ptr(out, np.uint64)
        n = C.c_uint64()
        if fn == "enc":
            rc = self.L.ukm_encode_kmers(self.h, pb, poff, n_rec, k, int(canonical), int(circular), po, cap,
                                         C.byref(n))
        else:
            rc = self.L.ukm_nthash(self.h, pb, poff, n_rec, k, int(canonical), int(circular), max_hash, po, cap,
                                   C.byref(n))
        _check(rc, n.value)
        return out[: n.value]

    def encode_kmers(self, bases, rec_off, k, canonical=True, circular=False, out=None):
        return self._windows("enc", bases, rec_off, k, canonical, circular, 0, out)

    def nthash(self, bases, rec_off, k, canonical=True, circular=False, max_hash=0, out=None):
        return self._windows("nt", bases, rec_off, k, canonical, circular, max_hash, out)

    def minimizer(self, bases, rec_off, k, w, circular=False, max_hash=0, with_pos=False, out=None, out_pos=None):
        """Minimizer sketch of every record (sketches.NewMinimizerSketch, count.go:316).  Returns the
        emitted canonical ntHash values in record/group order (and their window indices).  out / out_pos: the caller's
        arrays (out_pos as long as out; giving it implies with_pos)."""
        pb, nb, _ = _ptr(bases, np.uint8)
        poff, noff, _ = _ptr(rec_off, np.uint64)
        with_pos = with_pos or out_pos is not None
        if out is None:
            cap = nb
            out = _empty_like_kind(bases, cap, np.uint64)
            po = _ptr(out, np.uint64)[0]
        else:
            po, cap, _ = _ptr(out, np.uint64)
        pos = out_pos if out_pos is not None else (_empty_like_kind(bases, cap, np.uint64) if with_pos else None)
        pp, npos, _ = _ptr(pos, np.uint64) if with_pos else (None, 0, None)
        if out_pos is not None and npos < cap:
            raise ValueError("minimizer: out_pos is shorter than out")
        n = C.c_uint64()
        _check(self.L.ukm_minimizer(self.h, pb, poff, noff - 1, k, w, int(circular), max_hash, po, pp, cap,
                                    C.byref(n)), n.value)
        return (out[: n.value], pos[: n.value]) if with_pos else out[: n.value]

    def count(self, bases, rec_off, k, canonical=True, circular=False, hashed=False, max_hash=0, mode=UNIQUE, out=None):
        """`unikmer count -s` in one call (count.go:285-436,581): every window -> sort -> the distinct (`mode=UNIQUE`), repeated
        (`-d`: REPEATED) or singleton (`-u`: SINGLETON) set, sorted.  The windows stay on the device."""
        pb, nb, _ = _ptr(bases, np.uint8)
        poff, noff, _ = _ptr(rec_off, np.uint64)
        if out is None:
            cap = nb + 1
            if hashed and max_hash:
                cap = min(cap, int(nb * min(1.0, 3.0 * max_hash / float(1 << 64))) + (1 << 20))
            out = _empty_like_kind(bases, cap, np.uint64)
        po, cap, _ = _ptr(out, np.uint64)
        n = C.c_uint64()
        _check(self.L.ukm_count(self.h, pb, poff, noff - 1, int(k), int(canonical), int(circular), int(hashed), int(max_hash), int(mode), po,
                                cap, C.byref(n)), n.value)
        return out[: n.value]

    def max_hash(self, scale):
        return self.L.ukm_max_hash(scale)

    # ---- k-mers back to the genome ----
    def _coords(self, call, ref, dtypes, out_cap, given=None):
        """run call(pointers, cap, n) with caller-side outputs of `out_cap` entries; with out_cap None: a first guess, and
        the exact size the library reports (UKM_ERR_CAPACITY, n_out) for the one repeat.  given: the caller's own arrays,
        all of one length (that length is the capacity)"""
        if given is not None:
            out_cap = _ptr(given[0], dtypes[0])[1]
            assert len(given) == len(dtypes) and all(_ptr(o, dt)[1] == out_cap for o, dt in zip(given, dtypes))
        cap = (1 << 16) if out_cap is None else int(out_cap)
        for attempt in (0, 1):
            outs = list(given) if given is not None else [_empty_like_kind(ref, cap, dt) for dt in dtypes]
            n = C.c_uint64()
            rc = call([_ptr(o, dt)[0] for o, dt in zip(outs, dtypes)], cap, n)
            if rc == ERR_CAPACITY and out_cap is None and attempt == 0:
                cap = int(n.value)
                continue
            _check(rc, n.value)
            return tuple(o[: n.value] for o in outs)

    def locate(self, bases, rec_off, k, q_keys, circular=False, hashed=False, out_cap=None, outs=None):
        """`unikmer locate` (locate.go:141-289): every occurrence of every queried code.  Returns (q, rec, pos): index into
        q_keys, record index, window index in the record; queries in q_keys order (a code only where it first appears),
        a query's windows ascending."""
        pb, _, k1 = _ptr(bases, np.uint8)
        poff, noff, k2 = _ptr(rec_off, np.uint64)
        pq, nq, k3 = _ptr(q_keys, np.uint64)
        return self._coords(lambda o, cap, n: self.L.ukm_locate(self.h, pb, poff, noff - 1, int(k), int(circular), int(hashed), pq, nq,
                                                                o[0], o[1], o[2], cap, C.byref(n)),
                            bases, (np.uint64, np.uint32, np.uint64), out_cap, outs)

    def map(self, bases, rec_off, genome_off, k, set_keys, hashed=False, allow_multi=False, min_len=200, out_cap=None, outs=None):
        """`unikmer map` / `uniqs` at -x 0 -X 0 (map.go:116-491): regions covered by k-mers of the sorted set.  Returns
        (rec, start, end) per region, in record then position order.  genome_off groups records into genomes
        (None: every record its own genome)."""
        pb, _, k1 = _ptr(bases, np.uint8)
        poff, noff, k2 = _ptr(rec_off, np.uint64)
        if genome_off is None:
            genome_off = np.arange(noff, dtype=np.uint64)
        pg, ng, k3 = _ptr(genome_off, np.uint64)
        ps, ns, k4 = _ptr(set_keys, np.uint64)
        return self._coords(lambda o, cap, n: self.L.ukm_map(self.h, pb, poff, noff - 1, pg, ng - 1, int(k), int(hashed), ps, ns,
                                                             int(allow_multi), int(min_len), o[0], o[1], o[2], cap, C.byref(n)),
                            bases, (np.uint32, np.uint64, np.uint64), out_cap, outs)

    def map_gapped(self, bases, rec_off, genome_off, k, set_keys, hashed=False, circular=False, allow_multi=False, min_len=200,
                   max_gap_size=0, max_gap_num=0, out_cap=None, outs=None):
        """`unikmer map` / `uniqs` with -x max_gap_size, -X max_gap_num and --circular (map.go:298-490; the definition and the
        two deviations from the reference: include/unikmer_hip.h, ukm_map_gapped).  Returns (rec, start, end) per region, in
        record then start order; on circular records end may exceed the record's length.  max_gap_size = 0 on linear
        records is `map`."""
        pb, _, k1 = _ptr(bases, np.uint8)
        poff, noff, k2 = _ptr(rec_off, np.uint64)
        if genome_off is None:
            genome_off = np.arange(noff, dtype=np.uint64)
        pg, ng, k3 = _ptr(genome_off, np.uint64)
        ps, ns, k4 = _ptr(set_keys, np.uint64)
        return self._coords(lambda o, cap, n: self.L.ukm_map_gapped(self.h, pb, poff, noff - 1, pg, ng - 1, int(k), int(hashed), int(circular),
                                                                    ps, ns, int(allow_multi), int(min_len), int(max_gap_size),
                                                                    int(max_gap_num), o[0], o[1], o[2], cap, C.byref(n)),
                            bases, (np.uint32, np.uint64, np.uint64), out_cap, outs)

    # ---- which records belong to a set ----
    def screen(self, bases, rec_off, k, set_keys, set_taxids=None, canonical=True, circular=False, hashed=False, lca=None, outs=None):
        """Per record: (win, hit, lca) = its number of windows, the number of them whose value is in the sorted `set_keys`
        (every window counts), and the LCA of the hits' taxids (include/unikmer_hip.h: ukm_screen; 0 without a hit; needs a
        loaded taxonomy).  lca defaults to `set_taxids is not None`; without it the third value is None.  The windows are
        those of encode_kmers (hashed=False) / nthash (hashed=True) with the same canonical / circular.  outs: the caller's
        (win, hit, lca) arrays of n_rec uint32 each; an entry that is None is not computed and comes back as None."""
        pb, _, k1 = _ptr(bases, np.uint8)
        poff, noff, k2 = _ptr(rec_off, np.uint64)
        ps, ns, k3 = _ptr(set_keys, np.uint64)
        pt, nt, k4 = _ptr(set_taxids, np.uint32)
        n_rec = max(noff - 1, 0)
        if set_taxids is not None and nt != ns:
            raise ValueError("screen: set_taxids must be as long as set_keys")
        if lca is None:
            lca = set_taxids is not None
        if lca and set_taxids is None:
            raise ValueError("screen: lca needs set_taxids")
        if outs is None:
            outs = (_empty_like_kind(bases, n_rec, np.uint32), _empty_like_kind(bases, n_rec, np.uint32),
                    _empty_like_kind(bases, n_rec, np.uint32) if lca else None)
        elif len(outs) != 3 or any(o is not None and _ptr(o, np.uint32)[1] < n_rec for o in outs):
            raise ValueError("screen: outs must be (win, hit, lca) of at least n_rec items each (or None)")
        po = [None if o is None else (_ptr(o, np.uint32)[0] if n_rec else None) for o in outs]
        if po[2] is not None and ns == 0:
            pt = None   # (an empty set has no taxids to point at: every lca is 0)
        _check(self.L.ukm_screen(self.h, pb, poff, n_rec, int(k), int(canonical), int(circular), int(hashed), ps, pt, ns, po[0], po[1], po[2]))
        return tuple(None if o is None else o[:n_rec] for o in outs)

    # ---- record selection (grep / filter / sample): kept records in input order, taxids copied ----
    def _select(self, call, keys, taxids, bound, out, out_taxids):
        """taxids: an array (one per record), an int (the file's ONE taxid: only grep by taxid looks at it) or None"""
        pk, n, k1 = _ptr(keys, np.uint64)
        per_record = taxids is not None and not _is_file_taxid(taxids)
        pt, nt, k2 = _ptr(taxids if per_record else None, np.uint32)
        if per_record:
            assert nt == n
        cap = n if bound is None else bound(n)
        if out is None:
            out = _empty_like_kind(keys, cap, np.uint64)
        if per_record and out_taxids is None:
            out_taxids = _empty_like_kind(keys, cap, np.uint32)
        po, cap, _ = _ptr(out, np.uint64)
        pot, _, _ = _ptr(out_taxids if per_record else None, np.uint32)
        m = C.c_uint64()
        _check(call(pk, pt, n, po, pot, cap, C.byref(m)), m.value)
        return (out[: m.value], out_taxids[: m.value]) if per_record else out[: m.value]

    def grep(self, keys, queries=None, query_taxids=None, taxids=None, canonical_k=0, invert=False, out=None, out_taxids=None):
        """`unikmer grep` (grep.go:617-676): the records whose code is among `queries` -- or whose taxid is among
        `query_taxids` -- in input order, duplicates kept, each with its own taxid.  canonical_k in 1..32: every code is made
        canonical first (files that are neither canonical nor hashed).  taxids as an int: the file's one taxid."""
        if (queries is None) == (query_taxids is None):
            raise ValueError("grep: give exactly one of queries and query_taxids")
        pq, nq, k3 = _ptr(queries, np.uint64)
        pqt, nqt, k4 = _ptr(query_taxids, np.uint32)
        flags = (F_INVERT if invert else 0) | (F_QUERY_TAXID if query_taxids is not None else 0)
        ft = int(taxids) if _is_file_taxid(taxids) else 0
        return self._select(lambda pk, pt, n, po, pot, cap, m: self.L.ukm_grep(self.h, pk, pt, ft, n, int(canonical_k), pq, pqt,
                                                                               nq if queries is not None else nqt, flags, po, pot, cap, m),
                            keys, taxids, None, out, out_taxids)

    def filter(self, keys, k, taxids=None, threshold=15, window=7, penalty_s=3, penalty_d=1, invert=False, out=None, out_taxids=None):
        """`unikmer filter` (filter.go:181-221): drops the low-complexity k-mers (invert: keeps only them)"""
        return self._select(lambda pk, pt, n, po, pot, cap, m: self.L.ukm_filter(self.h, pk, pt, n, int(k), int(window), int(penalty_s),
                                                                                 int(penalty_d), int(threshold), F_INVERT if invert else 0,
                                                                                 po, pot, cap, m),
                            keys, taxids, None, out, out_taxids)

    def sample(self, keys, start=1, window=1, taxids=None, out=None, out_taxids=None):
        """`unikmer sample` (sample.go:134-148): record j (1-based) when j >= start and (j - start) % window == 0"""
        start, window = int(start), int(window)
        return self._select(lambda pk, pt, n, po, pot, cap, m: self.L.ukm_sample(self.h, pk, pt, n, start, window, po, pot, cap, m),
                            keys, taxids, (lambda n: (n - start) // window + 1 if start >= 1 and window >= 1 and n >= start else 0),
                            out, out_taxids)

    def rfilter(self, keys, f, taxids=None, out=None, out_taxids=None):
        """`unikmer rfilter` (rfilter.go:280-304): the records whose taxid passes the RankFilter `f`, in input order, each with
        its own taxid.  taxids as an int: the file's one taxid (a copy or an empty result)."""
        ft = int(taxids) if _is_file_taxid(taxids) else 0
        return self._select(lambda pk, pt, n, po, pot, cap, m: self.L.ukm_rfilter(self.h, pk, pt, ft, n, C.addressof(f), po, pot, cap, m),
                            keys, taxids, None, out, out_taxids)

    def tsplit(self, keys, taxids, out=None, group_taxids=None, group_off=None):
        """`unikmer tsplit` (tsplit.go:112-192): the records grouped by taxid, groups ascending, a group's codes in input
        order.  Returns (out_keys, group_taxids, group_off): group g is out_keys[group_off[g]:group_off[g + 1]].  Without
        the group arrays the number of groups is asked for first (the size query)."""
        pk, n, k1 = _ptr(keys, np.uint64)
        pt, nt, k2 = _ptr(taxids, np.uint32)
        assert taxids is None or nt == n
        g = C.c_uint64()
        out = _empty_like_kind(keys, n, np.uint64) if out is None else out

        def call(groups):
            po, cap, _ = _ptr(out if groups else None, np.uint64)
            pg, gcap, _ = _ptr(groups and groups[0], np.uint32)
            pf, fcap, _ = _ptr(groups and groups[1], np.uint64)
            # group_off holds one entry more than group_taxids: the capacity is what both arrays take
            return self.L.ukm_tsplit(self.h, pk, pt, n, po, cap if n else 0, pg, pf, min(gcap, max(fcap, 1) - 1), C.byref(g)), g.value
        (group_taxids, group_off), ng = _sized(call, None if group_taxids is None or group_off is None else (group_taxids, group_off),
                                               lambda m: (_empty_like_kind(keys, m, np.uint32), _empty_like_kind(keys, m + 1, np.uint64)))
        return out[:n], group_taxids[:ng], group_off[: ng + 1 if n else 0]

    # ---- .unik bodies (the bytes behind a file's header, inflated; layout: host/unik.hpp) ----
    def unik_decode(self, body, k, flags, taxid_bytes=0, with_taxids=True, out=None, out_taxids=None):
        """the records of a body: (keys, taxids), taxids None when the records carry none or with_taxids is False (the
        taxid bytes are skipped then).  Without `out` the number of records is asked for first (the size query)."""
        pb, nb, k1 = _ptr(body, np.uint8)
        tax = bool(flags & UNIK_INCLUDE_TAXID) and (with_taxids or out_taxids is not None)
        n = C.c_uint64()
        return _sized_records(lambda po, pot, cap: (self.L.ukm_unik_decode(self.h, pb, nb, int(k), int(flags), int(taxid_bytes), po, pot, cap,
                                                                           C.byref(n)), n.value), body, tax, out, out_taxids, nb == 0)

    def unik_encode(self, keys, k, flags, taxids=None, taxid_bytes=0, out=None):
        """the body unik::Writer writes for these records, as uint8.  Without `out` it is sized by unik_encode_bound."""
        pk, n, k1 = _ptr(keys, np.uint64)
        pt, nt, k2 = _ptr(taxids, np.uint32)
        assert taxids is None or nt == n
        if out is None:
            out = _empty_like_kind(keys, unik_encode_bound(n, k, flags, taxid_bytes), np.uint8)
        po, cap, _ = _ptr(out, np.uint8)
        m = C.c_uint64()
        _check(self.L.ukm_unik_encode(self.h, pk, pt, n, int(k), int(flags), int(taxid_bytes), po, cap if n else 0, C.byref(m)), m.value)
        return out[: m.value]

    # ---- deflate (the gzip writer behind a .unik body) ----
    def deflate(self, data, crc=0, final=False, gzip=False, out=None):
        """(fragment, crc): `data` (uint8) as a byte-aligned run of deflate blocks, Huffman coding only, where the input lives;
        crc in: zlib.crc32 of what precedes data in the caller's stream, out: of that followed by data.  final: the fragment
        ends the deflate stream; gzip: it is a complete gzip member.  Without `out` it is sized by deflate_bound."""
        pd, n, k1 = _ptr(data, np.uint8)
        flags = (DEFLATE_FINAL if final else 0) | (DEFLATE_GZIP if gzip else 0)
        m, c = C.c_uint64(), C.c_uint32(int(crc) & 0xFFFFFFFF)
        if out is None:
            out = _empty_like_kind(data, deflate_bound(n, final, gzip), np.uint8)
        po, cap, _ = _ptr(out, np.uint8)
        _check(self.L.ukm_deflate(self.h, pd, n, flags, po, cap, C.byref(m), C.byref(c)), m.value)
        return out[: m.value], int(c.value)

    # ---- inflate (the gzip reader in front of a .unik body) ----
    def inflate(self, data, crc=0, out=None):
        """(bytes_out, consumed, crc): the longest prefix of `data` (uint8: a raw deflate fragment that starts at a block
        boundary on a byte boundary) that is non-final blocks of literals -- what Context.deflate writes -- inflated where
        the input lives.  consumed: the bytes of data that prefix takes, always a block start on a byte boundary; go on from
        there with zlib.decompressobj(-15, zdict=<the last 32 KiB of output>).  consumed == 0 is no error: a stream with
        matches gives it.  crc in: zlib.crc32 of what precedes bytes_out in the caller's stream, out: of that followed by
        bytes_out.  Without `out` the size is asked for first; too small an `out`: CapacityError with .needed and
        .consumed."""
        pd, n, k1 = _ptr(data, np.uint8)
        m, used = C.c_uint64(), C.c_uint64()
        c = C.c_uint32(int(crc) & 0xFFFFFFFF)

        def call(o):
            po, cap, _ = _ptr(o, np.uint8)
            c.value = int(crc) & 0xFFFFFFFF
            return self.L.ukm_inflate(self.h, pd, n, 0, po, cap if o is not None else 0, C.byref(m), C.byref(used), C.byref(c)), m.value
        try:
            out, size = _sized(call, out, lambda need: _empty_like_kind(data, need, np.uint8))
        except CapacityError as e:
            e.consumed = int(used.value)
            raise
        return out[:size], int(used.value), int(c.value)

    # ---- k-mer text (`unikmer view` / `unikmer dump`) ----
    def view(self, keys, taxids=None, file_taxid=0, *, k, hashed=False, fmt=VIEW_KMER, out=None):
        """the text `unikmer view` prints for the records, as uint8 where the inputs live.  taxids None: every record carries
        file_taxid.  Without `out` the size is asked for first (the size query; VIEW_KMER of plain codes is n (k + 1))."""
        pk, n, k1 = _ptr(keys, np.uint64)
        pt, nt, k2 = _ptr(taxids, np.uint32)
        assert taxids is None or nt == n
        args = (int(file_taxid), n, int(k), int(bool(hashed)), int(fmt))
        m = C.c_uint64()

        def call(o):
            po, cap, _ = _ptr(o, np.uint8)
            return self.L.ukm_view(self.h, pk, pt, *args, po, cap if n else 0, C.byref(m)), m.value
        out, size = _sized(call, out, lambda need: _empty_like_kind(keys, need, np.uint8))
        return out[:size]

    def dump(self, text, *, k, flags=0, out=None, out_taxids=None):
        """the records of k-mer text (`unikmer dump`, the strict grammar of include/unikmer_hip.h): (keys, taxids), taxids None
        without DUMP_TAXID.  Without `out` the number of records is asked for first.  A line outside the grammar: FormatError
        with bad_off."""
        pb, nb, k1 = _ptr(text, np.uint8)
        tax = bool(flags & DUMP_TAXID)
        n, bad = C.c_uint64(), C.c_uint64()

        def call(po, pot, cap):
            rc = self.L.ukm_dump(self.h, pb, nb, int(k), int(flags), po, pot, cap, C.byref(n), C.byref(bad))
            if rc == ERR_FORMAT:
                try:
                    _check(rc)
                except FormatError as e:
                    e.bad_off = bad.value
                    raise
            return rc, n.value
        return _sized_records(call, text, tax, out, out_taxids, nb == 0)

    # ---- FASTA/Q text (the input of `unikmer count`) ----
    def fastx(self, text, *, fastq=False, last=True, out=None):
        """(bases, rec_off, hdr_off, consumed, stop): the longest prefix of `text` (uint8, starting at a record boundary)
        inside the device's FASTA / FASTQ grammar (include/unikmer_hip.h: ukm_fastx), parsed where the text lives.  bases:
        the kept sequence bytes; rec_off [n_rec + 1]: record i is bases[rec_off[i]:rec_off[i + 1]]; hdr_off [n_rec]: where
        record i's '>' / '@' stands in text; consumed: the bytes of text that prefix takes; stop: FASTX_STOP_*.  last=False:
        more text follows, the incomplete record at the end is left to the next call.  out: (bases, rec_off, hdr_off) arrays
        of the caller (rec_off one longer than hdr_off); without it the sizes are asked for first.  Too small: CapacityError
        with .needed = (bases, records)."""
        pt, n, k1 = _ptr(text, np.uint8)
        flags = (FASTX_FASTQ if fastq else 0) | (FASTX_LAST if last else 0)
        nb, nr, used = C.c_uint64(), C.c_uint64(), C.c_uint64()
        stop = C.c_int()

        def call(o):
            pb, bcap, _ = _ptr(o and o[0], np.uint8)
            pr, rcap, _ = _ptr(o and o[1], np.uint64)
            ph, hcap, _ = _ptr(o and o[2], np.uint64)
            cap = min(rcap - 1, hcap) if o is not None else 0
            return self.L.ukm_fastx(self.h, pt, n, flags, pb, bcap, pr, ph, max(cap, 0), C.byref(nb), C.byref(nr), C.byref(used), C.byref(stop))
        if out is None:
            rc = call(None)
            if rc != ERR_CAPACITY:
                _check(rc)
            out = (_empty_like_kind(text, nb.value, np.uint8), _empty_like_kind(text, nr.value + 1, np.uint64),
                   _empty_like_kind(text, nr.value, np.uint64))
        rc = call(out)
        if rc == ERR_CAPACITY:
            try:
                _check(rc)
            except CapacityError as e:
                e.needed = (int(nb.value), int(nr.value))
                e.consumed, e.stop = int(used.value), int(stop.value)
                raise
        _check(rc)
        return out[0][: nb.value], out[1][: nr.value + 1], out[2][: nr.value], int(used.value), int(stop.value)

    # ---- sort / scans ----
    def sort_u64(self, keys, key_bits=64):
        """In place; returns keys."""
        if not _is_torch(keys):
            assert isinstance(keys, np.ndarray) and keys.dtype == np.uint64 and keys.flags.c_contiguous
        p, n, _ = _ptr(keys, np.uint64)
        _check(self.L.ukm_sort_u64(self.h, p, n, key_bits))
        return keys

    def sort_pairs(self, keys, taxids, key_bits=64):
        if not _is_torch(keys):
            assert isinstance(keys, np.ndarray) and keys.dtype == np.uint64 and keys.flags.c_contiguous
            assert isinstance(taxids, np.ndarray) and taxids.dtype == np.uint32 and taxids.flags.c_contiguous
        pk, n, _ = _ptr(keys, np.uint64)
        pt, n2, _ = _ptr(taxids, np.uint32)
        assert n == n2
        _check(self.L.ukm_sort_pairs(self.h, pk, pt, n, key_bits))
        return keys, taxids

    def unique(self, keys, taxids=None, mode=UNIQUE, out=None, out_taxids=None):
        pk, n, k1 = _ptr(keys, np.uint64)
        pt, _, k2 = _ptr(taxids, np.uint32)
        cap = 2 * n if mode == REPEATED_CHUNK else n
        if out is None:
            out = _empty_like_kind(keys, cap, np.uint64)
        if taxids is not None and out_taxids is None:
            out_taxids = _empty_like_kind(keys, cap, np.uint32)
        po, cap, _ = _ptr(out, np.uint64)
        pot, _, _ = _ptr(out_taxids, np.uint32)
        m = C.c_uint64()
        _check(self.L.ukm_unique(self.h, pk, pt, n, mode, po, pot, cap, C.byref(m)), m.value)
        return (out[: m.value], out_taxids[: m.value]) if taxids is not None else out[: m.value]

    # ---- set operations ----
    def setop2(self, op, a, b, a_taxids=None, b_taxids=None, flags=0, out=None, out_taxids=None):
        """a_taxids / b_taxids: an array (one taxid per record), an int (ONE taxid for the whole file: the .unik
        header's global taxid -- nothing is expanded, the kernels take the scalar) or None"""
        pa, na, k1 = _ptr(a, np.uint64)
        pb, nb, k2 = _ptr(b, np.uint64)
        fa = int(a_taxids) if _is_file_taxid(a_taxids) else 0
        fb = int(b_taxids) if _is_file_taxid(b_taxids) else 0
        pta, _, k3 = _ptr(None if _is_file_taxid(a_taxids) else a_taxids, np.uint32)
        ptb, _, k4 = _ptr(None if _is_file_taxid(b_taxids) else b_taxids, np.uint32)
        tax = (a_taxids is not None and not (_is_file_taxid(a_taxids) and fa == 0)) or \
              (b_taxids is not None and not (_is_file_taxid(b_taxids) and fb == 0))
        bound = na + nb if op == OP_UNION else na
        if out is None:
            out = _empty_like_kind(a, bound, np.uint64)
        if tax and out_taxids is None:
            out_taxids = _empty_like_kind(a, bound, np.uint32)
        po, cap, _ = _ptr(out, np.uint64)
        pot, _, _ = _ptr(out_taxids, np.uint32)
        n = C.c_uint64()
        _check(self.L.ukm_setop2_ft(self.h, op, pa, pta, fa, na, pb, ptb, fb, nb, flags, po, pot, cap, C.byref(n)), n.value)
        return (out[: n.value], out_taxids[: n.value]) if tax else out[: n.value]

    def setop2_multi(self, a, b, ops=(OP_UNION, OP_INTER), a_taxids=None, b_taxids=None, flags=0, out=None, out_taxids=None):
        """Two or three operations of ONE pair from a single pass over a and b (ukm_setop2_multi): {op: result}, each
        entry what setop2(op, a, b, ...) returns -- the trimmed output, or (out, out_taxids) where taxids are present.
        ops: the operations wanted (OP_UNION / OP_INTER / OP_DIFF); plain codes and at least two of them run fused,
        everything else one pass per operation.  out / out_taxids: dicts {op: caller-owned buffer}; an operation without
        an entry gets a buffer of setop2's default size (na + nb for the union, na otherwise).  Too small:
        CapacityError with .needed = {op: records} for every requested operation."""
        ops = tuple(int(x) for x in ops)
        mask = 0
        for x in ops:
            mask |= (1 << x) if x >= 0 else 0
        pa, na, k1 = _ptr(a, np.uint64)
        pb, nb, k2 = _ptr(b, np.uint64)
        fa = int(a_taxids) if _is_file_taxid(a_taxids) else 0
        fb = int(b_taxids) if _is_file_taxid(b_taxids) else 0
        pta, _, k3 = _ptr(None if _is_file_taxid(a_taxids) else a_taxids, np.uint32)
        ptb, _, k4 = _ptr(None if _is_file_taxid(b_taxids) else b_taxids, np.uint32)
        tax = (a_taxids is not None and not (_is_file_taxid(a_taxids) and fa == 0)) or \
              (b_taxids is not None and not (_is_file_taxid(b_taxids) and fb == 0))
        out = dict(out or {})
        out_taxids = dict(out_taxids or {})
        po, pot, cap, n = (C.c_void_p * 3)(), (C.c_void_p * 3)(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        keep = []
        for x in ops:
            if not 0 <= x <= OP_DIFF:
                continue   # (the library refuses the mask)
            bound = na + nb if x == OP_UNION else na
            if out.get(x) is None:
                out[x] = _empty_like_kind(a, bound, np.uint64)
            if tax and out_taxids.get(x) is None:
                out_taxids[x] = _empty_like_kind(a, bound, np.uint32)
            p, c, ka = _ptr(out[x], np.uint64)
            pt, _, kb = _ptr(out_taxids.get(x), np.uint32)
            po[x], pot[x], cap[x] = p, pt, c
            keep += [ka, kb]
        rc = self.L.ukm_setop2_multi(self.h, mask, pa, pta, fa, na, pb, ptb, fb, nb, flags, po, pot, cap, n)
        if rc == ERR_CAPACITY:
            try:
                _check(rc)
            except CapacityError as e:
                e.needed = {x: int(n[x]) for x in ops}
                raise
        _check(rc)
        return {x: ((out[x][: n[x]], out_taxids[x][: n[x]]) if tax else out[x][: n[x]]) for x in ops}

    def stream_table(self, keys_list, taxids_list=None):
        """Prepared pointer / length tables of a set of streams, to be passed IN PLACE OF keys_list to union / inter / diff /
        common / merge_k any number of times (taxids_list is then ignored).  A host that keeps its decoded .unik streams on
        the device builds these arrays once per file set -- they are exactly the `keys` / `taxids` / `lens` arguments of the
        C ABI; building them from 1000 torch tensors costs this Python binding ~0.4 ms per call otherwise."""
        return StreamTable(self._nway_args(list(keys_list), taxids_list), keys_list[0] if len(keys_list) else np.empty(0, np.uint64))

    def _nway_args(self, keys_list, taxids_list):
        if isinstance(keys_list, StreamTable):
            return keys_list.args
        n = len(keys_list)
        # entries of taxids_list that are plain ints are FILE taxids (one value for every record of the stream): they go to
        # the C ABI's file_taxids[] as they are
        ft = None
        if taxids_list is not None and any(_is_file_taxid(t) for t in taxids_list):
            ft_np = np.array([int(t) if _is_file_taxid(t) else 0 for t in taxids_list], dtype=np.uint32)
            taxids_list = [None if _is_file_taxid(t) else t for t in taxids_list]
            ft = (ft_np, bool(ft_np.any()))
        tax0 = taxids_list is not None and any(t is not None for t in taxids_list)
        if n >= 64 and all(_is_torch(k) for k in keys_list) and (not tax0 or all(t is None or _is_torch(t) for t in taxids_list)):
            # many device tensors (a 1000-file fold): the tables are built with numpy, not element by element through
            # ctypes (1.5 ms of a 4 ms call went into that)
            assert all(k.is_contiguous() and k.element_size() == 8 for k in keys_list)
            lens_np = np.fromiter((k.numel() for k in keys_list), dtype=np.uint64, count=n)
            kp_np = np.fromiter((k.data_ptr() if k.numel() else 0 for k in keys_list), dtype=np.uint64, count=n)
            tp_np = None
            if tax0:
                assert all(t is None or (t.is_contiguous() and t.element_size() == 4 and t.numel() == k.numel())
                           for t, k in zip(taxids_list, keys_list))
                tp_np = np.fromiter((t.data_ptr() if (t is not None and t.numel()) else 0 for t in taxids_list), dtype=np.uint64, count=n)
            kp = (C.c_void_p * n).from_buffer(kp_np)
            tp = (C.c_void_p * n).from_buffer(tp_np) if tp_np is not None else None
            lens = (C.c_uint64 * n).from_buffer(lens_np)
            on_device = all(k.is_cuda for k in keys_list) and (not tax0 or all(t is None or t.is_cuda for t in taxids_list))
            return kp, tp, lens, n, tax0 or bool(ft and ft[1]), int(lens_np.sum()), [keys_list, taxids_list, kp_np, tp_np, lens_np, "device" if on_device else "host"], ft
        keep = []
        kp = (C.c_void_p * max(n, 1))()
        tp = (C.c_void_p * max(n, 1))()
        lens = (C.c_uint64 * max(n, 1))()
        tax = taxids_list is not None and any(t is not None for t in taxids_list)
        for i, k in enumerate(keys_list):
            p, ln, ka = _ptr(k, np.uint64)
            kp[i] = p
            lens[i] = ln
            keep.append(ka)
            if tax and taxids_list[i] is not None:
                pt, lt, kt = _ptr(taxids_list[i], np.uint32)
                assert lt == ln
                tp[i] = pt
                keep.append(kt)
        total = sum(int(lens[i]) for i in range(n))
        # (as on the path above: _nway looks at the last entry to see whether EVERY stream pointer is a device pointer)
        on_device = n > 0 and all(_is_torch(a) and a.is_cuda for a in keep if a is not None)
        keep.append("device" if on_device else "host")
        return kp, (tp if tax else None), lens, n, tax or bool(ft and ft[1]), total, keep, ft

    def _nway(self, which, keys_list, taxids_list, bound, extra, flags, out, out_taxids):
        kp, tp, lens, n, tax, total, keep, ft = self._nway_args(keys_list, taxids_list)
        pft = ft[0].ctypes.data if ft is not None else None
        if (len(keep) and isinstance(keep[-1], str) and keep[-1] == "device" and which != "merge"
                and not os.environ.get("UKM_PY_NO_DEVICE_FLAG")):
            flags |= F_DEVICE_STREAMS      # all inputs are CUDA tensors: the library need not classify 2 x n pointers
        ref = (keys_list.ref if isinstance(keys_list, StreamTable) else keys_list[0]) if n else np.empty(0, np.uint64)
        cap = bound(total, int(lens[0]) if n else 0)
        if out is None:
            out = _empty_like_kind(ref, cap, np.uint64)
        if tax and out_taxids is None:
            out_taxids = _empty_like_kind(ref, cap, np.uint32)
        po, cap, _ = _ptr(out, np.uint64)
        pot, _, _ = _ptr(out_taxids, np.uint32)
        m = C.c_uint64()
        kpp = C.cast(kp, C.POINTER(C.c_void_p))
        tpp = C.cast(tp, C.POINTER(C.c_void_p)) if tp is not None else None
        L = self.L
        if which == "union":
            rc = L.ukm_union_ft(self.h, kpp, tpp, pft, lens, n, flags, po, pot, cap, C.byref(m))
        elif which == "inter":
            rc = L.ukm_inter_ft(self.h, kpp, tpp, pft, lens, n, flags, po, pot, cap, C.byref(m))
        elif which == "diff":
            sf = extra
            psf = None
            if sf is not None:
                sf = np.ascontiguousarray(sf, dtype=np.uint8)
                psf = sf.ctypes.data
            rc = L.ukm_diff_ft(self.h, kpp, tpp, pft, lens, n, psf, flags, po, pot, cap, C.byref(m))
        elif which == "common":
            rc = L.ukm_common_ft(self.h, kpp, tpp, pft, lens, n, extra, flags, po, pot, cap, C.byref(m))
        else:
            mode, final_round = extra
            rc = L.ukm_merge_k_ft(self.h, kpp, tpp, pft, lens, n, mode, int(final_round), po, pot, cap, C.byref(m))
        _check(rc, m.value)
        return (out[: m.value], out_taxids[: m.value]) if tax else out[: m.value]

    def union(self, keys_list, taxids_list=None, out=None, out_taxids=None):
        return self._nway("union", keys_list, taxids_list, lambda t, f: t, None, 0, out, out_taxids)

    def inter(self, keys_list, taxids_list=None, mix_taxid=False, out=None, out_taxids=None):
        return self._nway("inter", keys_list, taxids_list, lambda t, f: f, None,
                          F_MIX_TAXID if mix_taxid else 0, out, out_taxids)

    def diff(self, keys_list, taxids_list=None, compare_taxid=False, sorted_flags=None, out=None,
             out_taxids=None):
        return self._nway("diff", keys_list, taxids_list, lambda t, f: f, sorted_flags,
                          F_CMP_TAXID if compare_taxid else 0, out, out_taxids)

    def common(self, keys_list, threshold, taxids_list=None, out=None, out_taxids=None):
        return self._nway("common", keys_list, taxids_list, lambda t, f: t, int(threshold), 0, out, out_taxids)

    def merge_k(self, keys_list, taxids_list=None, mode=PLAIN, final_round=True, out=None, out_taxids=None):
        return self._nway("merge", keys_list, taxids_list, lambda t, f: 2 * t, (mode, final_round), 0, out,
                          out_taxids)

    def pair_counts(self, keys_list, rows=None, out=None, sizes=True):
        """All-pairs shared code counts (ukm_pair_counts): counts[i][j] = the number of distinct codes streams i and j share,
        i < rows (default: all n streams, the full symmetric matrix), j < n; sizes[j] = the distinct codes of stream j.
        keys_list: numpy arrays or torch tensors (host or device, mixed), as for union; they need not be sorted or
        duplicate-free.  Returns (counts, sizes): counts a (rows, n) uint64 array on the host, or `out` (a contiguous array or
        tensor of rows * n 8-byte items, host or device) as the caller gave it; sizes an (n,) uint64 host array, the array or
        tensor passed as `sizes`, or None for sizes=False.  similarity.py turns the pair into Jaccard / containment / Mash."""
        kp, _, lens, n, _, _, keep, _ = self._nway_args(list(keys_list), None)
        rows = n if rows is None else int(rows)
        if out is None and 1 <= rows <= n:
            out = np.empty((rows, n), dtype=np.uint64)
        if sizes is True:
            sizes = np.empty(max(n, 1), dtype=np.uint64)[:n]
        elif sizes is False:
            sizes = None
        po, cap, _ = _ptr(out, np.uint64)
        ps, scap, _ = _ptr(sizes, np.uint64)
        if 1 <= rows <= n:
            assert cap == rows * n, "out holds %d items, the matrix has %d x %d" % (cap, rows, n)
            assert sizes is None or scap == n, "sizes holds %d items for %d streams" % (scap, n)
        _check(self.L.ukm_pair_counts(self.h, C.cast(kp, C.POINTER(C.c_void_p)), lens, n, rows, 0, po, ps))
        return out, sizes

    def common_threshold(self, nfiles, proportion=1.0, number=0):
        return self.L.ukm_common_threshold(nfiles, proportion, number)

    # ---- multi-GPU exchange through the C ABI (RCCL inside the library; dist.py is the torch.distributed twin) ----
    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * 128)()
        _check(load().ukm_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        assert len(uid) == 128
        _check(self.L.ukm_comm_init(self.h, nranks, rank, C.c_char_p(uid)))

    def comm_destroy(self):
        _check(self.L.ukm_comm_destroy(self.h))

    def comm_info(self):
        n, r = C.c_int(), C.c_int()
        _check(self.L.ukm_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def prefix_splitters(self, key_bits, nranks):
        sp = np.empty(nranks, dtype=np.uint64)
        _check(self.L.ukm_prefix_splitters(key_bits, nranks, sp.ctypes.data))
        return sp

    @staticmethod
    def shard_plan(nranks, rank, gathered):
        """the collective capacity decision of ukm_shard_exchange as a pure host function: gathered =
        [source rank][nranks slice sizes | out_cap of that rank].  Returns (recv_counts, n_out); raises CapacityError
        on EVERY rank when ANY rank's buffer is too small."""
        g = np.ascontiguousarray(gathered, dtype=np.uint64).reshape(nranks, nranks + 1)
        rc = np.zeros(nranks, dtype=np.uint64)
        m = C.c_uint64()
        _check(load().ukm_shard_plan(nranks, rank, g.ctypes.data, rc.ctypes.data, C.byref(m)))
        return rc, m.value

    @staticmethod
    def shard_splitters_plan(nranks, gathered, key_bits):
        """sampled splitters from the gathered words ([rank][1 + per_rank] = record count, samples): the pure host
        function behind ukm_shard_splitters, also used by unikmer_amd/dist.py.  Returns nranks + 1 Python ints."""
        g = np.ascontiguousarray(gathered, dtype=np.uint64).reshape(nranks, -1)
        out = np.zeros(nranks + 1, dtype=np.uint64)
        _check(load().ukm_shard_splitters_plan(nranks, g.shape[1] - 1, g.ctypes.data, int(key_bits), out.ctypes.data))
        sp = [int(x) for x in out]
        if key_bits < 64:
            sp[-1] = 1 << key_bits
        return sp

    def shard_splitters(self, keys_list, key_bits):
        """collective (RCCL communicator of this context): sampled splitters for the sorted files this rank holds"""
        kp, _, lens, n, _, _, keep, _ft = self._nway_args(list(keys_list), None)
        out = np.zeros(self.comm_info()[0] + 1, dtype=np.uint64)
        _check(self.L.ukm_shard_splitters(self.h, C.cast(kp, C.POINTER(C.c_void_p)), lens, n, int(key_bits), out.ctypes.data))
        sp = [int(x) for x in out]
        if key_bits < 64:
            sp[-1] = 1 << key_bits
        return sp

    def shard_counts(self, send_counts, has_taxids=None):
        """send_counts [nfiles][nranks] -> recv_counts [nfiles][nranks] (one all-gather + one host sync for all files).
        has_taxids [nfiles] (bools): which files this rank will exchange WITH taxids; the flags ride in the same gather and
        ranks that disagree about a file all raise (ukm_shard_counts_tax)."""
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        if sc.ndim == 1:
            sc = sc[None, :]
        rc = np.zeros_like(sc)
        if has_taxids is None:
            _check(self.L.ukm_shard_counts(self.h, sc.ctypes.data, sc.shape[0], rc.ctypes.data))
        else:
            ht = np.ascontiguousarray(has_taxids, dtype=np.uint8)
            assert ht.shape == (sc.shape[0],)
            _check(self.L.ukm_shard_counts_tax(self.h, sc.ctypes.data, sc.shape[0], ht.ctypes.data, rc.ctypes.data))
        return rc

    @staticmethod
    def shard_counts_plan(nranks, rank, gathered):
        """the decision of ukm_shard_counts_tax as a pure host function: gathered = [rank][nfiles * nranks sizes | nfiles
        flags (0 / 1 / 2 = not declared)] -> recv_counts [nfiles][nranks] of `rank`; raises when two ranks disagree"""
        g = np.ascontiguousarray(gathered, dtype=np.uint64)
        nfiles = g.shape[1] // (nranks + 1)
        assert g.shape == (nranks, nfiles * (nranks + 1))
        rc = np.zeros((nfiles, nranks), dtype=np.uint64)
        _check(load().ukm_shard_counts_plan(nranks, rank, nfiles, g.ctypes.data, rc.ctypes.data))
        return rc

    def shard_exchange(self, keys, send_counts, taxids=None, recv_counts=None):
        """all-to-all-v of the contiguous slices of one sorted stream; returns (keys, taxids | None, recv_counts).
        The receive sizes are learned first (ukm_shard_counts) and the output is sized from them: n_local x nranks is
        NOT a bound on what a rank receives (a rank with few local records may own a dense prefix range).  Callers
        that already hold the counts of many files (shard_counts) pass recv_counts and skip the per-file gather."""
        pk, n, k1 = _ptr(keys, np.uint64)
        pt, _, k2 = _ptr(taxids, np.uint32)
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        assert int(sc.sum()) == n
        rc = (np.ascontiguousarray(recv_counts, dtype=np.uint64) if recv_counts is not None
              else self.shard_counts(sc, [taxids is not None])[0])
        cap = max(1, int(rc.sum()))
        out = _empty_like_kind(keys, cap, np.uint64)
        out_t = _empty_like_kind(keys, cap, np.uint32) if taxids is not None else None
        po, _, _ = _ptr(out, np.uint64)
        pot, _, _ = _ptr(out_t, np.uint32)
        m = C.c_uint64()
        _check(self.L.ukm_shard_exchange_known(self.h, pk, pt, sc.ctypes.data, rc.ctypes.data, po, pot, cap, C.byref(m)))
        return out[: m.value], (out_t[: m.value] if out_t is not None else None), rc

    def partition_points(self, keys, splitters, out=None):
        """splitters (and out, the cuts) may be device tensors: the C ABI takes them where they are"""
        pk, n, k1 = _ptr(keys, np.uint64)
        sp = splitters if _is_torch(splitters) else np.ascontiguousarray(splitters, dtype=np.uint64)
        ps, ns, k2 = _ptr(sp, np.uint64)
        cuts = out if out is not None else _empty_like_kind(sp, ns, np.uint64)
        pc, nc, k3 = _ptr(cuts, np.uint64)
        assert nc >= ns
        _check(self.L.ukm_partition_points(self.h, pk, n, ps, ns, pc))
        return cuts[:ns]
