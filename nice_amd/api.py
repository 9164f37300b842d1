"""Host-side mirror of the reference's field-processing API over the C ABI.

Names, argument meaning and error behaviour follow
common/src/client_process_gpu.rs (GpuContext, process_range_detailed_gpu,
process_range_niceonly_gpu, process_detailed_gpu, process_niceonly_gpu) and
common/src/client_process.rs (process_range_detailed, process_range_niceonly,
which here run on the GPU through a default context -- the drop-in the
north star asks for).  All compute happens in libnice_hip.so.
"""
from __future__ import annotations

import array
import ctypes
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import _lib
from ._lib import check, lib
from .types import (DataToClient, DataToServer, FieldResults, FieldSize, NiceNumberSimple,
                    UniquesDistributionSimple)

CLIENT_VERSION = "3.2.15-mi355x"
MASK64 = (1 << 64) - 1


def _split(n: int):
    if n < 0 or n >> 128:
        raise ValueError("value must fit in u128")
    return n & MASK64, n >> 64


# pub const GPU_BATCH_SIZE / PROCESSING_CHUNK_SIZE (client_process_gpu.rs:54, 59)
def _const(name):
    try:
        return int(getattr(lib(), name)())
    except _lib.NiceLibraryError:
        return None


GPU_BATCH_SIZE = 50_000_000
PROCESSING_CHUNK_SIZE = 1_000_000


def get_base_range_u128(base: int) -> Optional[FieldSize]:
    """get_base_range_u128 (common/src/base_range.rs:43-54)."""
    a, b, c, d = (ctypes.c_uint64() for _ in range(4))
    rc = lib().nice_base_range(base, a, b, c, d)
    if rc < 0:
        raise OverflowError(f"base {base}: range does not fit in u128")
    if rc == 0:
        return None
    return FieldSize(a.value | (b.value << 64), c.value | (d.value << 64))


def get_near_miss_cutoff(base: int) -> int:
    """get_near_miss_cutoff (common/src/number_stats.rs:15-17)."""
    return int(lib().nice_near_miss_cutoff(base))


def gpu_supports_base(base: int) -> bool:
    return bool(lib().nice_gpu_supports_base(base))


def niceonly_fast_base(base: int) -> bool:
    """The base's niceonly fields inside its range run the compile-time kernels
    (square-survivor queue, `NiceonlyStats.square_ok` counted): every base with
    an FD kernel and a non-empty k = 2 stride table."""
    return bool(lib().nice_niceonly_fast_base(base))


@dataclass
class StrideTable:
    """StrideTable (common/src/stride_filter.rs:20-87), host-built by the library."""
    base: int
    k: int
    modulus: int
    valid_residues: List[int]

    @classmethod
    def new(cls, base: int, k: int) -> "StrideTable":
        m = ctypes.c_uint64()
        n = ctypes.c_size_t()
        check(lib().nice_stride_table(base, k, m, None, 0, n))
        buf = (ctypes.c_uint32 * max(n.value, 1))()
        check(lib().nice_stride_table(base, k, m, buf, n.value, n))
        return cls(base, k, m.value, list(buf[: n.value]))


def get_valid_ranges(range_: FieldSize, base: int, floor_size: int = 250,
                     filter: str = "reference") -> List[FieldSize]:
    """get_valid_ranges_recursive (common/src/msd_prefix_filter.rs:583-674);
    filter="sound": without Filter C (nice_msd_valid_ranges_ex)."""
    s, e = range_.range_start, range_.range_end
    f = _FILTERS[filter]
    n = ctypes.c_size_t()
    rc = lib().nice_msd_valid_ranges_ex(*_split(s), *_split(e), base, floor_size, f, None, 0, n)
    if rc not in (_lib.NICE_OK, _lib.NICE_ERR_CAPACITY):
        check(rc)
    buf = (ctypes.c_uint64 * (4 * max(n.value, 1)))()
    check(lib().nice_msd_valid_ranges_ex(*_split(s), *_split(e), base, floor_size, f, buf, n.value, n))
    return [FieldSize(buf[4 * i] | (buf[4 * i + 1] << 64), buf[4 * i + 2] | (buf[4 * i + 3] << 64))
            for i in range(n.value)]


def has_duplicate_msd_prefix(range_: FieldSize, base: int) -> bool:
    """has_duplicate_msd_prefix (common/src/msd_prefix_filter.rs:382-563)."""
    rc = lib().nice_msd_skippable(*_split(range_.range_start), *_split(range_.range_end), base)
    if rc < 0 or rc > 1:
        check(rc)
    return bool(rc)


@dataclass
class NiceonlyStats:
    ranges: int
    range_numbers: int
    candidates: int
    launches: int
    msd_seconds: float
    total_seconds: float
    # device MSD, in-range fast bases: candidates whose square alone has no
    # repeated digit (mod 2^32; 0 where not counted)
    square_ok: int = 0
    # the MSD recursion floor the field used (msd_floor="adaptive": the
    # adaptive floor's value at submit)
    msd_floor: int = 0
    # host MSD worker threads the field ran (0: the MSD ran on the device)
    msd_threads: int = 0
    # times the field re-ran with grown device lists
    reruns: int = 0
    # filter="sound": candidates the per-candidate prefix test rejected before
    # the square test (0 for the reference filter and where sound mode runs
    # without the test: run-time-base kernels, out-of-range fields, host MSD)
    prefix_rejected: int = 0


_FILTERS = {"reference": _lib.NICE_FILTER_REFERENCE, "sound": _lib.NICE_FILTER_SOUND}


def _stats(st) -> NiceonlyStats:
    """The stats of the niceonly field this thread collected last."""
    return NiceonlyStats(st.ranges, st.range_numbers, st.candidates, st.launches,
                         st.msd_seconds, st.total_seconds, st.square_ok, st.msd_floor,
                         st.msd_threads, st.reruns, int(lib().nice_niceonly_prefix_rejected()))


def host_threads() -> int:
    """std::thread::available_parallelism() as the library computes it (the
    affinity mask capped by the cgroup cpu.max quota): the host MSD pool's
    size when threads=0 (client_process_gpu.rs:598)."""
    return int(lib().nice_host_threads())


def adaptive_floor_step(floor: float, msd_seconds: float, total_seconds: float) -> float:
    """AdaptiveFloor::update's step (client_process_gpu.rs:130-157)."""
    return lib().nice_adaptive_floor_step(floor, msd_seconds, total_seconds)


def adaptive_floor() -> Tuple[float, int]:
    """The process-wide adaptive MSD floor and its warmup fields left
    (0xffffffff: pinned by NICE_GPU_MSD_FLOOR)."""
    f, w = ctypes.c_double(), ctypes.c_uint32()
    check(lib().nice_adaptive_floor(f, w))
    return f.value, w.value


@dataclass
class KernelStats:
    kernel_ms: float
    launches: int
    fd_kernel: bool
    numbers: int
    sib_lanes: int = 0   # sibling lanes of the FD kernel's last sibling launch (0: none)
    sib_stride: int = 0  # ... and its lane stride
    sib_grid: int = 0    # ... and the workgroups of its persistent sibling grid (0: rounds of workgroups)


@dataclass
class RangesStats:
    launches: int         # batch-kernel launches of the call
    fallback_ranges: int  # ranges run one by one as fields (not inside an FD base's valid range)
    numbers: int
    kernel_ms: float      # HIP events around the batch launches


@dataclass
class MapStats:
    launches: int          # kernel launches of the call
    fd_segments: int       # pieces run by the FD map kernel (one per limb layout and device)
    generic_segments: int  # pieces run by the generic per-n kernel
    fd_numbers: int
    generic_numbers: int
    kernel_ms: float       # HIP events around the launches (the slowest device)


@dataclass
class RangesNiceonlyStats:
    launches: int        # kernel launches of the call (at most two per device)
    fast_ranges: int     # ranges run by the base's compile-time kernel (square_ok counted)
    generic_ranges: int  # ranges run by the run-time-base test
    candidates: int      # summed over the ranges
    square_ok: int
    kernel_ms: float     # HIP events around the launches (the slowest device)


@dataclass
class RangesNiceonlyPrefixStats:
    prefix_ranges: int   # ranges the prefix test ran on
    launches: int        # mask-kernel launches (one per device that had such ranges)
    rejected: int        # candidates the test rejected, summed over the ranges
    mask_ms: float       # HIP events around the mask launch (the slowest device)


@dataclass
class MsdRangesStats:
    launches: int     # recursion kernel launches of the call (the sort's not counted)
    fused_roots: int  # roots run one workgroup per root
    level_roots: int  # roots run by the level BFS
    ranges: int       # summed over the roots
    numbers: int      # the numbers inside them
    kernel_ms: float  # HIP events around the recursion launches (the slowest device)
    order_ms: float   # ... and around the device sort of the records


class RangeBounds:
    """A range list as the library holds it: four u64 per range (start_lo,
    start_hi, end_lo, end_hi), what msd_ranges returns.  niceonly_ranges,
    detailed_ranges and msd_ranges take it as it is, with no loop over the
    ranges; indexing and iteration give (start, end) pairs."""

    def __init__(self, buf, n: int, roots=None):
        self.buf, self.n = buf, n
        self.roots = roots  # per range, the index of the root it came from (msd_ranges), or None

    def __len__(self):
        return self.n

    def _words(self):
        return memoryview(self.buf).cast("B").cast("Q")[:4 * self.n].tolist()

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.tolist()[i]
        if i < 0:
            i += self.n
        if not 0 <= i < self.n:
            raise IndexError(i)
        b = self.buf
        return (b[4 * i] | (b[4 * i + 1] << 64), b[4 * i + 2] | (b[4 * i + 3] << 64))

    def __iter__(self):
        return iter(self.tolist())

    def tolist(self):
        w = self._words()
        return [(w[i] | (w[i + 1] << 64), w[i + 2] | (w[i + 3] << 64)) for i in range(0, len(w), 4)]

    def part(self, i: int, j: int) -> "RangeBounds":
        """Ranges [i, j) as a RangeBounds of their own (one buffer copy)."""
        i, j = max(0, min(i, self.n)), max(0, min(j, self.n))
        raw = memoryview(self.buf).cast("B")[32 * i:32 * max(i, j)]
        buf = (ctypes.c_uint64 * max(4 * (j - i), 4))()
        ctypes.memmove(buf, bytes(raw), len(raw))
        return RangeBounds(buf, max(0, j - i), self.roots[i:j] if self.roots is not None else None)

    def root_list(self):
        return list(self.roots[:self.n]) if self.roots is not None else None

    def numbers(self) -> int:
        """The numbers inside the ranges, summed."""
        w = self._words()
        return sum(w[2::4]) - sum(w[0::4]) + ((sum(w[3::4]) - sum(w[1::4])) << 64)


def _pack_ranges(ranges):
    """(start, end) pairs or FieldSize -> the four-u64-per-range bounds array
    nice_msd_valid_ranges writes (a RangeBounds is that array already)."""
    if isinstance(ranges, RangeBounds):
        return ranges.buf, len(ranges)
    pairs = [(r.range_start, r.range_end) if isinstance(r, FieldSize) else (int(r[0]), int(r[1]))
             for r in ranges]
    if any(s < 0 or e < 0 or s >> 128 or e >> 128 for s, e in pairs):
        raise ValueError("value must fit in u128")
    if not pairs:
        flat = array.array("Q", [0, 0, 0, 0])
    elif max(e for _, e in pairs) <= MASK64 and max(s for s, _ in pairs) <= MASK64:
        # (hundreds of thousands of survey windows: strided copies instead of a Python loop per value)
        flat = array.array("Q", bytes(32 * len(pairs)))
        flat[0::4] = array.array("Q", [s for s, _ in pairs])
        flat[2::4] = array.array("Q", [e for _, e in pairs])
    else:
        flat = array.array("Q", [x for s, e in pairs for x in (s & MASK64, s >> 64, e & MASK64, e >> 64)])
    # (one buffer copy: filling a ctypes array element by element costs ~1 us per value)
    return (ctypes.c_uint64 * len(flat)).from_buffer_copy(flat), len(pairs)


def _with_room(call, cap, bufs):
    """call(*bufs(cap), cap, n_out) -> rc, again with the room it asks for while
    it answers NICE_ERR_CAPACITY; returns (the buffers, n_out)."""
    while True:
        out, n = bufs(cap), ctypes.c_size_t()
        rc = call(*out, cap, n)
        if rc == _lib.NICE_ERR_CAPACITY and n.value > cap:  # retry only with more room
            cap = n.value
            continue
        check(rc)
        return out, n.value


def _cpu_out(cap: int):
    return (_lib.nice_number * max(cap, 1))()


def _list_bufs(cap):
    """A number list and its range indices."""
    return _cpu_out(cap), (ctypes.c_uint32 * cap)()


def _ranges_result(hist, nb, nrows, out, idx, n):
    full = memoryview(hist).cast("B").cast("Q").tolist()
    rows = [full[i * nb:(i + 1) * nb] for i in range(nrows)]
    return rows, [(out[i].number_lo | (out[i].number_hi << 64), out[i].num_uniques, idx[i])
                  for i in range(n)]


class GpuContext:
    """GpuContext (client_process_gpu.rs:196-306).  `devices` extends the
    reference's single ordinal: a field is sharded across the listed GPUs."""

    def __init__(self, devices: Sequence[int] | int = 0):
        if isinstance(devices, int):
            devices = [devices]
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        check(lib().nice_ctx_create(arr, len(devices), ctypes.byref(h)))
        self._h = h
        self.devices = list(devices)
        # Reused host output buffer (grown on NICE_ERR_CAPACITY): allocating a
        # zeroed 64K-entry ctypes array per call cost ~0.1 ms of host time.
        self._out = None
        self._out_cap = 0
        self._hist = {}

    @classmethod
    def new(cls, device_ordinal: int = 0) -> "GpuContext":
        return cls([device_ordinal])

    def close(self):
        if getattr(self, "_h", None):
            lib().nice_ctx_destroy(self._h)
            self._h = None

    def synchronize(self):
        """Wait until every stream of this context is idle (nice_ctx_synchronize)."""
        check(lib().nice_ctx_synchronize(self._h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _out_buf(self, cap):
        """The reused list buffer, as _with_room's buffers: a 1-tuple."""
        if cap > self._out_cap:
            self._out = ((_lib.nice_number * cap)(),)
            self._out_cap = cap
        return self._out

    def set_kernel_timing(self, enable: bool):
        """HIP-event timing of later detailed fields (default on; off saves two
        runtime calls per field, and kernel_stats().kernel_ms reads 0)."""
        check(lib().nice_ctx_set_kernel_timing(self._h, 1 if enable else 0))

    def kernel_stats(self, device_index: int = 0) -> KernelStats:
        s = _lib.nice_kernel_stats()
        check(lib().nice_last_kernel_stats(self._h, device_index, s))
        return KernelStats(s.kernel_ms, s.launches, bool(s.fd_kernel), s.numbers, s.sib_lanes, s.sib_stride,
                           s.sib_grid)

    # -- detailed -------------------------------------------------------------
    def detailed_raw(self, start: int, end: int, base: int, cap: int = 0):
        """Histogram (base+1 bins) and near-miss list [(n, u)] ascending."""
        hist = self._hist.get(base)
        if hist is None:
            hist = self._hist[base] = (ctypes.c_uint64 * (base + 1))()
        (out,), n = _with_room(lambda *a: lib().nice_process_range_detailed(
            self._h, *_split(start), *_split(end), base, hist, *a), max(cap, self._out_cap, 1024), self._out_buf)
        return list(hist), [(out[i].number_lo | (out[i].number_hi << 64), out[i].num_uniques)
                            for i in range(n)]

    def detailed_submit(self, start: int, end: int, base: int) -> int:
        """Enqueue a detailed field and return at once (a ticket for
        detailed_collect); at most three fields in flight per context."""
        t = ctypes.c_int()
        check(lib().nice_detailed_submit(self._h, *_split(start), *_split(end), base, t))
        return t.value

    def detailed_collect(self, ticket: int, base: int, cap: int = 0):
        """(hist, near-misses) of a submitted field, as detailed_raw returns."""
        hist = self._hist.get(base)
        if hist is None:
            hist = self._hist[base] = (ctypes.c_uint64 * (base + 1))()
        (out,), n = _with_room(lambda *a: lib().nice_detailed_collect(self._h, ticket, hist, *a),
                               max(cap, self._out_cap, 1024), self._out_buf)
        return list(hist), [(out[i].number_lo | (out[i].number_hi << 64), out[i].num_uniques)
                            for i in range(n)]

    # -- batched detailed ranges ------------------------------------------------
    def detailed_ranges(self, ranges, base: int, sum: bool = False, cap: int = 0):
        """Many (small) ranges in one call (nice_process_ranges_detailed):
        `ranges` holds (start, end) pairs or FieldSize.  Returns (rows,
        [(n, u, range_index)]): rows[i] is range i's histogram (base+1 bins) --
        with sum=True one row, the sum over the ranges -- and the list is each
        range's near-misses ascending, in range order.  In-range ranges of an
        FD base share one kernel launch per limb layout; see ranges_stats()."""
        bounds, n_ranges = _pack_ranges(ranges)
        nb = base + 1
        hist = (ctypes.c_uint64 * (nb * (1 if sum else max(n_ranges, 1))))()
        flags = _lib.NICE_RANGES_SUM if sum else _lib.NICE_RANGES_PER_RANGE
        (out, idx), n = _with_room(lambda *a: lib().nice_process_ranges_detailed(
            self._h, base, bounds, n_ranges, flags, hist, *a), max(cap, 1024), _list_bufs)
        return _ranges_result(hist, nb, 1 if sum else n_ranges, out, idx, n)

    def ranges_stats(self) -> "RangesStats":
        """Statistics of this context's last detailed_ranges call."""
        s = _lib.nice_ranges_stats()
        check(lib().nice_last_ranges_stats(self._h, s))
        return RangesStats(s.launches, s.fallback_ranges, s.numbers, s.kernel_ms)

    # -- the per-number map ------------------------------------------------------
    def unique_map(self, start: int, end: int, base: int, out=None):
        """The unique-digit count of n^2 and n^3 of every n in [start, end), one
        byte per number (nice_unique_map; at most 2^32 numbers).  With out=None
        the range is sharded over the context's GPUs and returned as a
        numpy.uint8 array.  With `out` a contiguous torch.uint8 tensor on one
        of the context's GPUs, at least end - start long (any storage offset),
        the map is written in place through its data_ptr() and `out` is
        returned.  The call returns only after the library's own stream has
        finished writing, so the caller's current torch stream -- any stream --
        may use the tensor straight away; work already queued on `out` by the
        caller must have finished before the call.  (torch and the library
        share one HIP runtime only when torch was imported, and found the GPU,
        before the library was first loaded -- bench.py's order; the other way
        round torch sees no device and there is no such tensor to pass.)
        bincount of the map is the detailed histogram of the range; see
        map_stats() for what ran."""
        size = end - start
        if out is None:
            import numpy as np
            buf = np.empty(max(size, 0), dtype=np.uint8)
            check(lib().nice_unique_map(self._h, *_split(start), *_split(end), base, buf.ctypes.data or None,
                                        buf.size, _lib.NICE_MAP_HOST, 0))
            return buf
        import torch
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_cuda and out.dim() == 1
                and out.is_contiguous()):
            raise ValueError("out must be a contiguous one-dimensional torch.uint8 tensor on a GPU")
        if out.device.index not in self.devices:
            raise ValueError(f"out lives on {out.device}, which is not one of the context's devices")
        # (the producer of `out`'s current contents, if any, is the caller's:
        # the library's stream does not wait for torch's)
        torch.cuda.current_stream(out.device).synchronize()
        check(lib().nice_unique_map(self._h, *_split(start), *_split(end), base, out.data_ptr() or None,
                                    out.numel(), _lib.NICE_MAP_DEVICE, self.devices.index(out.device.index)))
        return out

    def map_stats(self) -> "MapStats":
        """Statistics of this context's last unique_map call."""
        s = _lib.nice_map_stats()
        check(lib().nice_last_map_stats(self._h, s))
        return MapStats(s.launches, s.fd_segments, s.generic_segments, s.fd_numbers, s.generic_numbers,
                        s.kernel_ms)

    # -- batched niceonly ranges ------------------------------------------------
    def niceonly_ranges(self, ranges, base: int, stride_k: int = 0, cap: int = 0):
        """Many ranges in one call (nice_process_ranges_niceonly): `ranges`
        holds (start, end) pairs or FieldSize, e.g. what get_valid_ranges
        returns.  No MSD filter runs: every stride candidate of every range is
        tested.  Returns (candidates, square_ok, [(n, range_index)]): per range
        its stride candidates and how many have a repeat-free square (counted
        for a niceonly fast base's ranges inside its valid range on the k = 2
        table, else 0), and each range's nice numbers ascending, in range
        order.  See ranges_niceonly_stats()."""
        bounds, n_ranges = _pack_ranges(ranges)
        return _niceonly_ranges_call(
            lambda *a: lib().nice_process_ranges_niceonly(self._h, base, bounds, n_ranges, stride_k, *a),
            n_ranges, cap)

    def niceonly_ranges_ex(self, ranges, base: int, stride_k: int = 0, prefix_test: bool = False, cap: int = 0):
        """niceonly_ranges with options (nice_process_ranges_niceonly_ex).
        prefix_test=True runs the sound filter's per-candidate prefix test per
        range, where the field path runs it (a niceonly fast base, k = 2, the
        range inside the valid range): a mask kernel makes each range's mask
        of the common leading digits of n^2 and n^3, and the candidate kernel
        rejects against it ahead of the square test.  Returns (candidates,
        square_ok, prefix_rejected, [(n, range_index)]): candidates as
        niceonly_ranges counts them, prefix_rejected the rejected ones per
        range (0 where the test does not run), square_ok the KEPT candidates
        with a repeat-free square, the list the kept candidates that pass.
        prefix_test=False is niceonly_ranges with an all-zero third list.
        See ranges_niceonly_stats() and ranges_niceonly_prefix_stats()."""
        bounds, n_ranges = _pack_ranges(ranges)
        opts = _ranges_niceonly_opts(stride_k, prefix_test)
        return _niceonly_ranges_ex_call(
            lambda *a: lib().nice_process_ranges_niceonly_ex(self._h, base, bounds, n_ranges, opts, *a),
            n_ranges, cap)

    def ranges_niceonly_prefix_stats(self) -> "RangesNiceonlyPrefixStats":
        """The prefix test's part of this context's last niceonly_ranges(_ex) call."""
        s = _lib.nice_ranges_niceonly_prefix_stats()
        check(lib().nice_last_ranges_niceonly_prefix(self._h, s))
        return RangesNiceonlyPrefixStats(s.prefix_ranges, s.launches, s.rejected, s.mask_ms)

    def ranges_niceonly_stats(self) -> "RangesNiceonlyStats":
        """Statistics of this context's last niceonly_ranges call."""
        s = _lib.nice_ranges_niceonly_stats()
        check(lib().nice_last_ranges_niceonly_stats(self._h, s))
        return RangesNiceonlyStats(s.launches, s.fast_ranges, s.generic_ranges, s.candidates, s.square_ok,
                                   s.kernel_ms)

    # -- the device MSD recursion's range list ----------------------------------
    def msd_ranges(self, roots, base: int, floor_size: int = 250, filter: str = "reference", cap: int = 0):
        """The MSD recursion's surviving ranges of many roots in one call
        (nice_msd_ranges): `roots` holds (start, end) pairs, FieldSize or a
        RangeBounds, e.g. chunk_roots(start, end, chunk) -- then the list is
        the one that field's niceonly run tests.  Each root's answer is
        get_valid_ranges(root, base, floor_size, filter).  Returns (bounds,
        counts): a RangeBounds (the roots' answers concatenated in root order,
        bounds.roots the root index per range) that niceonly_ranges and
        detailed_ranges take unchanged, and the number of ranges per root.
        See msd_ranges_stats()."""
        rb, n_roots = _pack_ranges(roots)
        return _msd_ranges_call(
            lambda *a: lib().nice_msd_ranges(self._h, base, rb, n_roots, floor_size, _FILTERS[filter], *a),
            n_roots, cap)

    def msd_ranges_stats(self) -> "MsdRangesStats":
        """Statistics of this context's last msd_ranges call."""
        s = _lib.nice_msd_ranges_stats()
        check(lib().nice_last_msd_ranges_stats(self._h, s))
        return MsdRangesStats(s.launches, s.fused_roots, s.level_roots, s.ranges, s.numbers, s.kernel_ms,
                              s.order_ms)

    # -- niceonly -------------------------------------------------------------
    def niceonly_raw(self, start: int, end: int, base: int, msd_floor: int = 0,
                     chunk_size: int = 0, threads: int = 0, stride_k: int = 0,
                     msd_where: str = "auto", cap: int = 0, deal_stride: int = 0,
                     deal_offset: int = 0, filter: str = "reference"):
        """Nice numbers of [start, end) ascending, and NiceonlyStats.  With
        deal_stride N > 1 only the field's chunks c with c % N == deal_offset
        are processed (rank deal_offset of an N-way job, nice_amd/dist.py).
        filter="reference" is the reference's MSD filter bit for bit, Filter C
        included, which can drop numbers it has not ruled out; filter="sound"
        leaves Filter C out and tests each candidate against its own low
        digits instead (NICE_FILTER_SOUND, include/nice_hip.h): a complete
        answer, with NiceonlyStats.prefix_rejected."""
        opts = self._nice_opts(msd_floor, chunk_size, threads, stride_k, msd_where, deal_stride,
                               deal_offset, filter)
        st = _lib.nice_niceonly_stats()
        (out,), n = _with_room(lambda *a: lib().nice_process_range_niceonly_ex(
            self._h, *_split(start), *_split(end), base, opts, *a, st),
            max(cap, self._out_cap, 1024), self._out_buf)
        return [out[i].number_lo | (out[i].number_hi << 64) for i in range(n)], _stats(st)

    @staticmethod
    def _nice_opts(msd_floor=0, chunk_size=0, threads=0, stride_k=0, msd_where="auto",
                   deal_stride=0, deal_offset=0, filter="reference"):
        where = {"auto": 0, "host": 1, "device": 2}[msd_where]
        if filter not in _FILTERS:
            raise ValueError(f"filter must be one of {sorted(_FILTERS)}")
        if msd_floor == "adaptive":  # client_process_gpu.rs:96-184
            msd_floor = _lib.NICE_MSD_FLOOR_ADAPTIVE
        return _lib.nice_niceonly_opts(msd_floor, chunk_size, threads, stride_k, where,
                                       deal_stride, deal_offset, _FILTERS[filter])

    def niceonly_submit(self, start: int, end: int, base: int, **opts) -> int:
        """Enqueue a niceonly field (options as niceonly_raw) and return a
        ticket for niceonly_collect."""
        t = ctypes.c_int()
        check(lib().nice_niceonly_submit(self._h, *_split(start), *_split(end), base,
                                         self._nice_opts(**opts), t))
        return t.value

    def niceonly_collect(self, ticket: int, cap: int = 0):
        """(nice numbers, NiceonlyStats) of a submitted field."""
        st = _lib.nice_niceonly_stats()
        (out,), n = _with_room(lambda *a: lib().nice_niceonly_collect(self._h, ticket, *a, st),
                               max(cap, self._out_cap, 1024), self._out_buf)
        return [out[i].number_lo | (out[i].number_hi << 64) for i in range(n)], _stats(st)

    # -- both modes of one field ---------------------------------------------
    def both_raw(self, det_range, nice_range, base: int, **nice_opts):
        """Detailed of det_range and niceonly of nice_range (either None to
        skip), one after the other on this context's stream.  Returns
        ((hist, near_misses), (nice, stats)); BothModes runs the two at once."""
        det = self.detailed_raw(*det_range, base) if det_range else (None, [])
        nice = self.niceonly_raw(*nice_range, base, **nice_opts) if nice_range else ([], None)
        return det, nice

    def debug_unique_counts(self, ns: Sequence[int], base: int) -> List[int]:
        arr = (ctypes.c_uint64 * (2 * max(len(ns), 1)))()
        for i, n in enumerate(ns):
            arr[2 * i], arr[2 * i + 1] = _split(n)
        out = (ctypes.c_uint32 * max(len(ns), 1))()
        check(lib().nice_debug_unique_counts(self._h, arr, len(ns), base, out))
        return list(out[: len(ns)])

    def debug_unique_fast(self, ns: Sequence[int], base: int) -> List[int]:
        """Unique-digit counts by the niceonly kernel's in-range limb path
        (radix_fast.hpp); every n must lie in the base's valid range."""
        arr = (ctypes.c_uint64 * (2 * max(len(ns), 1)))()
        for i, n in enumerate(ns):
            arr[2 * i], arr[2 * i + 1] = _split(n)
        out = (ctypes.c_uint32 * max(len(ns), 1))()
        check(lib().nice_debug_unique_fast(self._h, arr, len(ns), base, out))
        return list(out[: len(ns)])

    def debug_cube_count(self, ns: Sequence[int], base: int) -> List[int]:
        """What the niceonly kernels' cube pass compares with the base: the
        digit-union count of n^2 and n^3, 0 when n^2 repeats a digit (LDS pair
        table for b <= 64, VALU above); every n in the base's valid range."""
        arr = (ctypes.c_uint64 * (2 * max(len(ns), 1)))()
        for i, n in enumerate(ns):
            arr[2 * i], arr[2 * i + 1] = _split(n)
        out = (ctypes.c_uint32 * max(len(ns), 1))()
        check(lib().nice_debug_cube_count(self._h, arr, len(ns), base, out))
        return list(out[: len(ns)])

    def debug_is_nice(self, ns: Sequence[int], base: int) -> List[bool]:
        arr = (ctypes.c_uint64 * (2 * max(len(ns), 1)))()
        for i, n in enumerate(ns):
            arr[2 * i], arr[2 * i + 1] = _split(n)
        out = (ctypes.c_uint32 * max(len(ns), 1))()
        check(lib().nice_debug_is_nice(self._h, arr, len(ns), base, out))
        return [bool(x) for x in out[: len(ns)]]


class BothModes:
    """Detailed and niceonly of one field at the same time on one GPU.

    Each mode gets its own context, i.e. its own HIP stream, and the niceonly
    pass is driven from a worker thread (ctypes releases the GIL for the
    call), so its launch-latency-bound MSD levels and candidate kernel run
    beside the detailed kernel instead of after it: the b40 1e9 bench step
    goes from 2.63 to 2.48 ms (scripts/overlap_probe.py).  Same results as
    GpuContext.both_raw, which runs the two in sequence."""

    def __init__(self, device: int = 0, det_ctx: Optional[GpuContext] = None,
                 nice_ctx: Optional[GpuContext] = None):
        self.det = det_ctx if det_ctx is not None else GpuContext([device])
        self.nice = nice_ctx if nice_ctx is not None else GpuContext([device])
        self._own_nice = nice_ctx is None
        self._go = threading.Event()
        self._done = threading.Event()
        self._job = None
        self._res = None
        self._closed = False
        self._thread = threading.Thread(target=self._serve, name="nice-niceonly", daemon=True)
        self._thread.start()

    def _serve(self):
        while True:
            self._go.wait()
            self._go.clear()
            if self._closed:
                return
            args, kw = self._job
            try:
                self._res = (True, self.nice.niceonly_raw(*args, **kw))
            except BaseException as e:  # re-raised on the calling thread
                self._res = (False, e)
            self._done.set()

    def kernel_stats(self, device_index: int = 0) -> KernelStats:
        """The detailed pass's kernel statistics."""
        return self.det.kernel_stats(device_index)

    def detailed_raw(self, *a, **kw):
        return self.det.detailed_raw(*a, **kw)

    def niceonly_raw(self, *a, **kw):
        return self.nice.niceonly_raw(*a, **kw)

    def both_raw(self, det_range, nice_range, base: int, **nice_opts):
        if self._closed:
            raise RuntimeError("BothModes is closed")
        if not nice_range:
            return (self.det.detailed_raw(*det_range, base) if det_range else (None, [])), ([], None)
        self._job = ((*nice_range, base), nice_opts)
        self._done.clear()
        self._go.set()
        try:
            det = self.det.detailed_raw(*det_range, base) if det_range else (None, [])
        finally:
            self._done.wait()
        ok, nice = self._res
        self._res = None
        if not ok:
            raise nice
        return det, nice

    def close(self):
        if not self._closed:
            self._closed = True
            self._go.set()
            self._thread.join()
            if self._own_nice:
                self.nice.close()


def process_range_detailed_gpu(ctx: GpuContext, range_: FieldSize, base: int) -> FieldResults:
    """process_range_detailed_gpu (client_process_gpu.rs:812-897)."""
    hist, lst = ctx.detailed_raw(range_.range_start, range_.range_end, base)
    return FieldResults(
        distribution=[UniquesDistributionSimple(i, hist[i]) for i in range(1, base + 1)],
        nice_numbers=[NiceNumberSimple(n, u) for n, u in lst])


def process_range_niceonly_gpu(ctx: GpuContext, range_: FieldSize, base: int,
                               **opts) -> FieldResults:
    """process_range_niceonly_gpu (client_process_gpu.rs:515-557)."""
    lst, _ = ctx.niceonly_raw(range_.range_start, range_.range_end, base, **opts)
    return FieldResults(distribution=[], nice_numbers=[NiceNumberSimple(n, base) for n in lst])


def process_detailed_gpu(ctx: GpuContext, claim: DataToClient, username: str) -> DataToServer:
    """process_detailed_gpu (client_process_gpu.rs:907-922)."""
    r = process_range_detailed_gpu(ctx, claim.field(), claim.base)
    return DataToServer(claim.claim_id, username, CLIENT_VERSION, r.distribution, r.nice_numbers)


def process_niceonly_gpu(ctx: GpuContext, claim: DataToClient, username: str) -> DataToServer:
    """process_niceonly_gpu (client_process_gpu.rs:924-941)."""
    r = process_range_niceonly_gpu(ctx, claim.field(), claim.base)
    return DataToServer(claim.claim_id, username, CLIENT_VERSION, None, r.nice_numbers)


_default_ctx: Optional[GpuContext] = None
_default_lock = threading.Lock()


def default_context() -> GpuContext:
    global _default_ctx
    with _default_lock:
        if _default_ctx is None:
            _default_ctx = GpuContext(0)
        return _default_ctx


def process_range_detailed(range_: FieldSize, base: int) -> FieldResults:
    """Drop-in for process_range_detailed (client_process.rs:150-191), on the GPU."""
    return process_range_detailed_gpu(default_context(), range_, base)


def process_range_niceonly(range_: FieldSize, base: int,
                           stride_table: Optional[StrideTable] = None) -> FieldResults:
    """Drop-in for process_range_niceonly (client_process.rs:439-465), on the GPU,
    with the CPU path's candidate set (MSD floor 250 over the whole range, stride
    table k from `stride_table`, default 2)."""
    k = stride_table.k if stride_table is not None else 2
    size = range_.range_size
    return process_range_niceonly_gpu(default_context(), range_, base, stride_k=k,
                                      chunk_size=min(size, (1 << 64) - 1))


def process_range_detailed_cpu(range_: FieldSize, base: int, threads: int = 1) -> FieldResults:
    """process_range_detailed (client_process.rs:150-191) on the host cores
    (nice_cpu_process_range_detailed): no device, for callers without a GPU.
    threads = 1 is the reference's single-threaded call."""
    hist = (ctypes.c_uint64 * (base + 1))()
    (out,), n = _with_room(lambda *a: lib().nice_cpu_process_range_detailed(
        *_split(range_.range_start), *_split(range_.range_end), base, threads, hist, *a),
        1024, lambda cap: (_cpu_out(cap),))
    return FieldResults(
        distribution=[UniquesDistributionSimple(i, hist[i]) for i in range(1, base + 1)],
        nice_numbers=[NiceNumberSimple(out[i].number_lo | (out[i].number_hi << 64), out[i].num_uniques)
                      for i in range(n)])


def unique_map_cpu(start: int, end: int, base: int, threads: int = 1):
    """GpuContext.unique_map on the host cores (nice_cpu_unique_map): no
    device.  Returns a numpy.uint8 array."""
    import numpy as np
    buf = np.empty(max(end - start, 0), dtype=np.uint8)
    check(lib().nice_cpu_unique_map(*_split(start), *_split(end), base, threads, buf.ctypes.data or None, buf.size))
    return buf


def detailed_ranges_cpu(ranges, base: int, sum: bool = False, threads: int = 1):
    """GpuContext.detailed_ranges on the host cores
    (nice_cpu_process_ranges_detailed): no device."""
    bounds, n_ranges = _pack_ranges(ranges)
    nb = base + 1
    hist = (ctypes.c_uint64 * (nb * (1 if sum else max(n_ranges, 1))))()
    flags = _lib.NICE_RANGES_SUM if sum else _lib.NICE_RANGES_PER_RANGE
    (out, idx), n = _with_room(lambda *a: lib().nice_cpu_process_ranges_detailed(
        base, bounds, n_ranges, flags, threads, hist, *a), 1024, _list_bufs)
    return _ranges_result(hist, nb, 1 if sum else n_ranges, out, idx, n)


def _ranges_field_results(rows, lst, base: int) -> List[FieldResults]:
    per = [[] for _ in rows]
    for n, u, i in lst:
        per[i].append(NiceNumberSimple(n, u))
    return [FieldResults(distribution=[UniquesDistributionSimple(i, row[i]) for i in range(1, base + 1)],
                         nice_numbers=nn) for row, nn in zip(rows, per)]


def process_ranges_detailed_gpu(ctx: GpuContext, ranges, base: int) -> List[FieldResults]:
    """process_range_detailed_gpu for every range of `ranges`, in one batched
    call (GpuContext.detailed_ranges)."""
    return _ranges_field_results(*ctx.detailed_ranges(ranges, base), base)


def process_ranges_detailed_cpu(ranges, base: int, threads: int = 1) -> List[FieldResults]:
    """process_range_detailed_cpu for every range of `ranges`."""
    return _ranges_field_results(*detailed_ranges_cpu(ranges, base, threads=threads), base)


def _niceonly_ranges_call(call, n_ranges: int, cap: int):
    """call(candidates, square_ok, out, out_range, cap, n_out) -> rc, retried
    with room on NICE_ERR_CAPACITY."""
    cand = (ctypes.c_uint64 * max(n_ranges, 1))()
    sq = (ctypes.c_uint32 * max(n_ranges, 1))()
    (out, idx), n = _with_room(lambda *a: call(cand, sq, *a), max(cap, 1024), _list_bufs)
    return (list(cand[:n_ranges]), list(sq[:n_ranges]),
            [(out[i].number_lo | (out[i].number_hi << 64), idx[i]) for i in range(n)])


def niceonly_ranges_cpu(ranges, base: int, stride_k: int = 0, threads: int = 1, cap: int = 0):
    """GpuContext.niceonly_ranges on the host cores
    (nice_cpu_process_ranges_niceonly): no device.  square_ok is counted for
    every range."""
    bounds, n_ranges = _pack_ranges(ranges)
    return _niceonly_ranges_call(
        lambda *a: lib().nice_cpu_process_ranges_niceonly(base, bounds, n_ranges, stride_k, threads, *a),
        n_ranges, cap)


def _ranges_niceonly_opts(stride_k: int, prefix_test):
    # (an integer passes through as it is, so that the library judges it)
    pt = int(prefix_test) if not isinstance(prefix_test, bool) else (
        _lib.NICE_RANGES_PREFIX_ON if prefix_test else _lib.NICE_RANGES_PREFIX_OFF)
    return _lib.nice_ranges_niceonly_opts(stride_k, pt)


def _niceonly_ranges_ex_call(call, n_ranges: int, cap: int):
    """call(candidates, square_ok, prefix_rejected, out, out_range, cap, n_out)
    -> rc, retried with room on NICE_ERR_CAPACITY."""
    cand = (ctypes.c_uint64 * max(n_ranges, 1))()
    sq = (ctypes.c_uint32 * max(n_ranges, 1))()
    rej = (ctypes.c_uint64 * max(n_ranges, 1))()
    (out, idx), n = _with_room(lambda *a: call(cand, sq, rej, *a), max(cap, 1024), _list_bufs)
    return (list(cand[:n_ranges]), list(sq[:n_ranges]), list(rej[:n_ranges]),
            [(out[i].number_lo | (out[i].number_hi << 64), idx[i]) for i in range(n)])


def niceonly_ranges_ex_cpu(ranges, base: int, stride_k: int = 0, prefix_test: bool = False, threads: int = 1,
                           cap: int = 0):
    """GpuContext.niceonly_ranges_ex on the host cores
    (nice_cpu_process_ranges_niceonly_ex): no device.  The prefix test runs on
    the same ranges as on the GPU; square_ok is counted for every range."""
    bounds, n_ranges = _pack_ranges(ranges)
    opts = _ranges_niceonly_opts(stride_k, prefix_test)
    return _niceonly_ranges_ex_call(
        lambda *a: lib().nice_cpu_process_ranges_niceonly_ex(base, bounds, n_ranges, opts, threads, *a),
        n_ranges, cap)


def _msd_ranges_call(call, n_roots: int, cap: int):
    """call(out, out_root, counts, cap, n_out) -> rc, retried with room on
    NICE_ERR_CAPACITY."""
    counts = (ctypes.c_uint64 * max(n_roots, 1))()
    (out, idx), n = _with_room(lambda o, r, *a: call(o, r, counts, *a), max(cap, 4096),
                               lambda c: ((ctypes.c_uint64 * (4 * c))(), (ctypes.c_uint32 * c)()))
    return RangeBounds(out, n, idx), list(counts[:n_roots])


def msd_ranges_cpu(roots, base: int, floor_size: int = 250, filter: str = "reference", threads: int = 1,
                   cap: int = 0):
    """GpuContext.msd_ranges on the host cores (nice_cpu_msd_ranges): the host
    recursion root by root, no device."""
    rb, n_roots = _pack_ranges(roots)
    return _msd_ranges_call(
        lambda *a: lib().nice_cpu_msd_ranges(base, rb, n_roots, floor_size, _FILTERS[filter], threads, *a),
        n_roots, cap)


def msd_ranges_plan(roots, base: int, floor_size: int = 250, n_devices: int = 1):
    """nice_debug_msd_ranges_plan: per root (index, group, device, batch);
    group 1 is one workgroup per root, 0 the level BFS.  No device."""
    rb, n_roots = _pack_ranges(roots)
    n = ctypes.c_size_t()
    buf = (ctypes.c_uint64 * (4 * max(n_roots, 1)))()
    check(lib().nice_debug_msd_ranges_plan(base, rb, n_roots, floor_size, n_devices, buf, n_roots, n))
    w = list(buf[:4 * n.value])
    return [tuple(w[i:i + 4]) for i in range(0, len(w), 4)]


def chunk_roots(start: int, end: int, chunk_size: int = 0) -> RangeBounds:
    """The roots of a field's chunk grid, as a niceonly field's device MSD takes
    them: chunks of chunk_size anchored at `start`, the last one ragged;
    chunk_size 0 is the reference client's rule (client/src/main.rs:158-168),
    which the field path uses by default.  msd_ranges of these roots is the
    range list that field's niceonly run tests."""
    if not 0 <= start < end or end >> 128:
        raise ValueError("the field must be non-empty and fit in u128")
    if chunk_size == 0:
        mult = -(-(end - start) // (1_000_000 * 100_000))
        chunk_size = 1_000_000 * max(1, min(mult, 1000))
    n = -(-(end - start) // chunk_size)
    if max(end, start) <= MASK64:
        flat = array.array("Q", bytes(32 * n))
        flat[0::4] = array.array("Q", range(start, end, chunk_size))
        flat[2::4] = array.array("Q", list(range(start + chunk_size, end, chunk_size)) + [end])
    else:
        flat = array.array("Q", [x for a in range(start, end, chunk_size) for b in (min(a + chunk_size, end),)
                                 for x in (a & MASK64, a >> 64, b & MASK64, b >> 64)])
    return RangeBounds((ctypes.c_uint64 * len(flat)).from_buffer_copy(flat), n)


def _ranges_niceonly_results(cand, lst, base: int) -> List[FieldResults]:
    per = [[] for _ in cand]
    for n, i in lst:
        per[i].append(NiceNumberSimple(n, base))
    return [FieldResults(distribution=[], nice_numbers=nn) for nn in per]


def process_ranges_niceonly_gpu(ctx: GpuContext, ranges, base: int, stride_k: int = 0) -> List[FieldResults]:
    """One FieldResults per range of `ranges`, from one batched call
    (GpuContext.niceonly_ranges): the ranges are tested as given, with no MSD
    filter in front."""
    cand, _, lst = ctx.niceonly_ranges(ranges, base, stride_k)
    return _ranges_niceonly_results(cand, lst, base)


def process_ranges_niceonly_cpu(ranges, base: int, stride_k: int = 0, threads: int = 1) -> List[FieldResults]:
    """process_ranges_niceonly_gpu on the host cores."""
    cand, _, lst = niceonly_ranges_cpu(ranges, base, stride_k, threads)
    return _ranges_niceonly_results(cand, lst, base)


def process_range_niceonly_cpu(range_: FieldSize, base: int,
                               stride_table: Optional[StrideTable] = None,
                               threads: int = 1, filter: str = "reference") -> FieldResults:
    """process_range_niceonly (client_process.rs:439-465) on the host cores
    (nice_cpu_process_range_niceonly_ex): MSD floor 250 over the whole range,
    stride table k from `stride_table` (default 2); filter="sound" runs the
    MSD recursion without Filter C."""
    k = stride_table.k if stride_table is not None else 2
    (out,), n = _with_room(lambda *a: lib().nice_cpu_process_range_niceonly_ex(
        *_split(range_.range_start), *_split(range_.range_end), base, k, threads, _FILTERS[filter], *a),
        256, lambda cap: (_cpu_out(cap),))
    return FieldResults(distribution=[], nice_numbers=[
        NiceNumberSimple(out[i].number_lo | (out[i].number_hi << 64), base) for i in range(n)])
