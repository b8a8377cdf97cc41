"""Device-side decoder objects over the C ABI (torch tensors as device memory, HIP streams).

These are the building blocks of the reference-compatible classes
(:mod:`.discrete_LDPC_decoder`, :mod:`.discrete_LDPC_decoder_irreg`,
:mod:`.min_sum_decoder_irreg`, :mod:`.bp_decoder_irreg`). PyTorch is only plumbing:
allocation, streams and ``torch.distributed``; every decode runs the HIP kernels of
``libibldpc.so`` and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .graph import EdgeGraph, build_graph
from .tables import IBTables

_DT_IB = {torch.uint8: _lib.IBL_U8, torch.int32: _lib.IBL_I32}
_DT_FL = {torch.float32: _lib.IBL_F32, torch.float64: _lib.IBL_F64}
_DT_ANY = {torch.uint8: _lib.IBL_U8, torch.int32: _lib.IBL_I32, torch.float32: _lib.IBL_F32,
           torch.float64: _lib.IBL_F64}


def _require_gpu(device) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the LDPC decoders run only on the GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"decoder device must be a HIP (cuda) device, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _stream_ptr(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _check_tensor(t: torch.Tensor, dev: torch.device, n_rows: int, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device != dev:
        raise ValueError(f"{name} must be a tensor on {dev}")
    if t.dim() != 2 or t.shape[0] != n_rows or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{n_rows}][B] tensor, got {tuple(t.shape)}")


class Graph:
    """A code graph uploaded to one device (``ibl_graph``)."""

    def __init__(self, H_or_graph, device=None):
        self.device = _require_gpu(device)
        self.edges: EdgeGraph = H_or_graph if isinstance(H_or_graph, EdgeGraph) else build_graph(H_or_graph)
        g = self.edges
        L = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(L.ibl_graph_create(g.n_v, g.n_c, np.ascontiguousarray(g.csr_indptr, np.int32),
                                      np.ascontiguousarray(g.csr_cols, np.int32), self.device.index,
                                      ctypes.byref(h)), "ibl_graph_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().ibl_graph_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None


class IBDecoder:
    """Information-bottleneck lookup-table decoder (``ibl_ib``) for up to ``max_batch`` codewords.

    ``path`` (fast path only): "auto" (the fused on-chip kernel when the code fits in LDS), "passes"
    (one launch per check / variable pass) or "fused" (raises when the code does not fit); both give
    identical results (``ibl_ib_set_path``). ``fused`` tells which one decodes run. ``fold`` switches the per-pass
    path's degree-2 variable fold (``ibl_ib_set_fold``; ``folded`` = variables it folds, results identical),
    ``composite`` the composite final step of its check chains (``ibl_ib_set_composite``; results identical),
    ``vn_composite`` that of its variable chains (``ibl_ib_set_vn_composite``; results identical)."""

    _PATHS = {"auto": _lib.IBL_PATH_AUTO, "passes": _lib.IBL_PATH_PASSES, "fused": _lib.IBL_PATH_FUSED}

    def __init__(self, graph: Graph, tables: IBTables, match: bool, max_batch: int, force_generic: bool = False,
                 path: str = "auto", fold: bool = True, composite: bool = True, vn_composite: bool = True):
        self.graph = graph
        self.tables = tables
        self.match = bool(match)
        self.max_batch = int(max_batch)
        self.device = graph.device
        tb = tables
        cn = np.ascontiguousarray(tb.cn, np.int32)
        vn = np.ascontiguousarray(tb.vn, np.int32)
        mc = np.ascontiguousarray(tb.match_cn if tb.match_cn is not None else np.zeros(1), np.int32)
        mv = np.ascontiguousarray(tb.match_vn if tb.match_vn is not None else np.zeros(1), np.int32)
        h = ctypes.c_void_p()
        L = _lib.load()
        _lib.check(L.ibl_ib_create(graph.handle, tb.Tc, tb.T, tb.imax, cn, cn.size, vn, vn.size, mc, mc.size,
                                   mv, mv.size, int(self.match), self.max_batch,
                                   _lib.IBL_FLAG_FORCE_GENERIC if force_generic else 0, ctypes.byref(h)),
                   "ibl_ib_create")
        self._h = h
        self.fast_path = bool(L.ibl_ib_path(h))
        if path not in self._PATHS:
            raise ValueError(f"path must be one of {sorted(self._PATHS)}")
        _lib.check(L.ibl_ib_set_path(h, self._PATHS[path]), "ibl_ib_set_path")
        if not fold:
            self.fold = False
        if not composite:
            self.composite = False
        if not vn_composite:
            self.vn_composite = False

    @property
    def fused(self) -> bool:
        f = ctypes.c_int32()
        _lib.check(_lib.load().ibl_ib_path_in_use(self._h, ctypes.byref(f)), "ibl_ib_path_in_use")
        return bool(f.value)

    @property
    def small_batch(self) -> int:
        """Largest batch the small-batch kernels decode (``ibl_ib_small_batch``; 0 = off)."""
        n = ctypes.c_int32()
        _lib.check(_lib.load().ibl_ib_small_batch(self._h, ctypes.byref(n)), "ibl_ib_small_batch")
        return int(n.value)

    @small_batch.setter
    def small_batch(self, max_b: int) -> None:
        _lib.check(_lib.load().ibl_ib_set_small_batch(self._h, int(max_b)), "ibl_ib_set_small_batch")

    @property
    def folded(self) -> int:
        """Degree-2 variables the per-pass fast path folds into the check pass (``ibl_ib_folded``)."""
        f = ctypes.c_int32()
        _lib.check(_lib.load().ibl_ib_folded(self._h, ctypes.byref(f)), "ibl_ib_folded")
        return int(f.value)

    @property
    def fold(self) -> bool:
        """Whether per-pass decodes fold (``ibl_ib_set_fold``; on by default, a no-op when ``folded`` is 0)."""
        return getattr(self, "_fold", True)

    @fold.setter
    def fold(self, on: bool) -> None:
        _lib.check(_lib.load().ibl_ib_set_fold(self._h, int(bool(on))), "ibl_ib_set_fold")
        self._fold = bool(on)

    @property
    def composite(self) -> int:
        """Check degree whose chains the per-pass fast path ends in the composite table step (``ibl_ib_composite``);
        0: none planned for this code, or switched off."""
        d = ctypes.c_int32()
        _lib.check(_lib.load().ibl_ib_composite(self._h, ctypes.byref(d)), "ibl_ib_composite")
        return int(d.value)

    @composite.setter
    def composite(self, on: bool) -> None:
        _lib.check(_lib.load().ibl_ib_set_composite(self._h, int(bool(on))), "ibl_ib_set_composite")

    @property
    def vn_composite(self) -> int:
        """Variable degree whose chains the per-pass fast path ends in the composite table step
        (``ibl_ib_vn_composite``), for the list its variable pass walks now (``fold``); 0: none planned, or off."""
        d = ctypes.c_int32()
        _lib.check(_lib.load().ibl_ib_vn_composite(self._h, ctypes.byref(d)), "ibl_ib_vn_composite")
        return int(d.value)

    @vn_composite.setter
    def vn_composite(self, on: bool) -> None:
        _lib.check(_lib.load().ibl_ib_set_vn_composite(self._h, int(bool(on))), "ibl_ib_set_vn_composite")

    def fused_ncw(self, B: int) -> int:
        """Codewords per workgroup the fused kernel decodes a batch of ``B`` with (8, or 4 for half
        groups; 0 when the fused kernel is not in use) — ``ibl_ib_fused_ncw``."""
        n = ctypes.c_int32()
        _lib.check(_lib.load().ibl_ib_fused_ncw(self._h, int(B), ctypes.byref(n)), "ibl_ib_fused_ncw")
        return int(n.value)

    def decode(self, ch: torch.Tensor, out: Optional[torch.Tensor] = None, out_dtype=torch.int32,
               early_stop=True, iters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode ``ch`` ([N][B] cluster ids, uint8/int32, on the decoder's device). ``early_stop``: True (the
        reference's stop, when the whole batch's syndrome is zero; ``iters`` receives one count), False, or
        ``"codeword"``: every codeword stops on its own and ``iters`` (int32 device tensor of at least B entries, or
        None) receives each one's count (``ibl_ib_decode_each``; fused kernel only, :class:`_lib.IBLError`
        otherwise)."""
        each = isinstance(early_stop, str)
        if each and early_stop != "codeword":
            raise ValueError('early_stop must be True, False or "codeword"')
        n = self.graph.edges.n_v
        _check_tensor(ch, self.device, n, "channel values")
        if ch.dtype not in _DT_IB:
            raise ValueError("channel values must be uint8 or int32")
        B = ch.shape[1]
        if out is None:
            out = torch.empty((n, B), dtype=out_dtype, device=self.device)
        _check_tensor(out, self.device, n, "output")
        if out.dtype not in _DT_IB or out.shape[1] != B:
            raise ValueError("output must be uint8/int32 [N][B]")
        it_ptr = None
        if iters is not None:
            if iters.dtype != torch.int32 or iters.device != self.device or iters.numel() < 1:
                raise ValueError("iters must be an int32 device tensor")
            if each and (iters.numel() < B or not iters.is_contiguous()):
                raise ValueError("iters must be a contiguous int32 device tensor of at least B entries")
            it_ptr = iters.data_ptr()
        if each:
            _lib.check(_lib.load().ibl_ib_decode_each(self._h, ch.data_ptr(), _DT_IB[ch.dtype], B, out.data_ptr(),
                                                      _DT_IB[out.dtype], it_ptr, _stream_ptr(self.device)),
                       "ibl_ib_decode_each")
            return out
        _lib.check(_lib.load().ibl_ib_decode(self._h, ch.data_ptr(), _DT_IB[ch.dtype], B, out.data_ptr(),
                                             _DT_IB[out.dtype], int(bool(early_stop)), it_ptr,
                                             _stream_ptr(self.device)), "ibl_ib_decode")
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().ibl_ib_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None


class FloatDecoder:
    """Float min-sum (kind=0) / BP (kind=1) decoder (``ibl_float``); precision fp32 or fp64.

    ``path``: "auto" (the fused on-chip kernel when the code fits in LDS), "passes" (one launch per
    check / variable pass) or "fused" (raises when the code does not fit); both give identical
    results (``ibl_float_set_path``). ``fused`` tells which one decodes run.

    ``alpha`` / ``beta`` (min-sum only): normalised / offset min-sum, every check magnitude becomes
    ``max(alpha * m - beta, 0)`` as two rounded operations (include/ibldpc.h "Corrected min-sum"); 0 < alpha <= 1,
    beta >= 0. The default (1, 0) is plain min-sum; ``correction`` returns the pair. ``kind=1`` with any other
    value raises ``ValueError``.

    Check degrees up to 32, variable degrees up to 16 (:class:`_lib.IBLError`, ``IBL_EUNSUPPORTED``, otherwise); a
    code with a check of degree above 16 makes a *wide* decoder (:attr:`wide`), every path and stop included."""

    _PATHS = {"auto": _lib.IBL_PATH_AUTO, "passes": _lib.IBL_PATH_PASSES, "fused": _lib.IBL_PATH_FUSED}

    def __init__(self, graph: Graph, kind: int, imax: int, max_batch: int, precision=torch.float32,
                 llr_max: float = 150.0, path: str = "auto", alpha: float = 1.0, beta: float = 0.0):
        self.graph = graph
        self.kind = int(kind)
        self.imax = int(imax)
        self.max_batch = int(max_batch)
        self.precision = precision
        self.device = graph.device
        corrected = not (float(alpha) == 1.0 and float(beta) == 0.0)
        if corrected and self.kind != _lib.IBL_MINSUM:
            raise ValueError("alpha / beta correct min-sum (kind=0) only")
        h = ctypes.c_void_p()
        if corrected:
            _lib.check(_lib.load().ibl_float_create_corrected(graph.handle, float(alpha), float(beta), self.imax,
                                                              float(llr_max), _DT_FL[precision], self.max_batch,
                                                              ctypes.byref(h)), "ibl_float_create_corrected")
        else:
            _lib.check(_lib.load().ibl_float_create(graph.handle, self.kind, self.imax, float(llr_max),
                                                    _DT_FL[precision], self.max_batch, ctypes.byref(h)),
                       "ibl_float_create")
        self._h = h
        if path not in self._PATHS:
            raise ValueError(f"path must be one of {sorted(self._PATHS)}")
        _lib.check(_lib.load().ibl_float_set_path(h, self._PATHS[path]), "ibl_float_set_path")

    @property
    def correction(self):
        """``(alpha, beta)`` of a min-sum decoder (``ibl_float_correction``; (1.0, 0.0) is plain min-sum)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.load().ibl_float_correction(self._h, ctypes.byref(a), ctypes.byref(b)), "ibl_float_correction")
        return float(a.value), float(b.value)

    @property
    def fused(self) -> bool:
        f = ctypes.c_int32()
        _lib.check(_lib.load().ibl_float_path_in_use(self._h, ctypes.byref(f)), "ibl_float_path_in_use")
        return bool(f.value)

    def fused_geometry(self, B: int):
        """``(ngroups, grid)`` the fused kernel decodes a batch of ``B`` with: groups of 4 fp32 / 2 fp64
        codewords and workgroups launched (workgroup w takes groups w, w + grid, ...); ``(0, 0)`` when the
        fused kernel is not in use — ``ibl_float_fused_geometry``."""
        n, g = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().ibl_float_fused_geometry(self._h, int(B), ctypes.byref(n), ctypes.byref(g)),
                   "ibl_float_fused_geometry")
        return int(n.value), int(g.value)

    @property
    def small_batch(self) -> int:
        """Largest batch the small-batch float kernels decode (``ibl_float_small_batch``; 0 = off)."""
        n = ctypes.c_int32()
        _lib.check(_lib.load().ibl_float_small_batch(self._h, ctypes.byref(n)), "ibl_float_small_batch")
        return int(n.value)

    @small_batch.setter
    def small_batch(self, max_b: int) -> None:
        _lib.check(_lib.load().ibl_float_set_small_batch(self._h, int(max_b)), "ibl_float_set_small_batch")

    @property
    def folded(self) -> int:
        """Degree-2 variables the per-pass path folds into the check pass (``ibl_float_folded``)."""
        f = ctypes.c_int32()
        _lib.check(_lib.load().ibl_float_folded(self._h, ctypes.byref(f)), "ibl_float_folded")
        return int(f.value)

    @property
    def wide(self) -> bool:
        """Whether the code has a check of degree above 16 (up to 32: DVB-S2 rates 4/5 to 9/10, 5G NR base graph 1),
        so that the check passes and the fused kernel run their wide forms (``ibl_float_is_wide``). Variable
        degrees stay at most 16."""
        w = ctypes.c_int32()
        _lib.check(_lib.load().ibl_float_is_wide(self._h, ctypes.byref(w)), "ibl_float_is_wide")
        return bool(w.value)

    def input_violations(self, raise_on_error: bool = True) -> int:
        """Channel LLRs of this decoder's decodes since the last call (on any stream) that broke the
        precondition (NaN; BP fp64 also |x| > 709.089, BP fp32 also +-inf): synchronises the device and clears
        the count (``ibl_float_input_check``). Raises :class:`_lib.IBLError` when there were any, unless
        ``raise_on_error`` is False."""
        v = ctypes.c_int32()
        rc = _lib.load().ibl_float_input_check(self._h, ctypes.byref(v), _stream_ptr(self.device))
        if raise_on_error:
            _lib.check(rc, "ibl_float_input_check")
        return int(v.value)

    def decode(self, llr: torch.Tensor, out: Optional[torch.Tensor] = None, out_dtype=None,
               early_stop=True, iters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``early_stop``: True (the reference's stop, when the whole batch's syndrome is zero; ``iters`` receives
        one count), False, or ``"codeword"``: every codeword stops on its own and ``iters`` (int32 device tensor of
        at least B entries, or None) receives each one's count (``ibl_float_decode_each``; fused kernel only,
        :class:`_lib.IBLError` otherwise)."""
        each = isinstance(early_stop, str)
        if each and early_stop != "codeword":
            raise ValueError('early_stop must be True, False or "codeword"')
        n = self.graph.edges.n_v
        _check_tensor(llr, self.device, n, "channel LLRs")
        if llr.dtype not in _DT_FL:
            raise ValueError("channel LLRs must be float32 or float64")
        B = llr.shape[1]
        if out is None:
            out = torch.empty((n, B), dtype=out_dtype or self.precision, device=self.device)
        _check_tensor(out, self.device, n, "output")
        if out.dtype not in _DT_FL or out.shape[1] != B:
            raise ValueError("output must be float32/float64 [N][B]")
        it_ptr = None
        if iters is not None:
            if iters.dtype != torch.int32 or iters.device != self.device or iters.numel() < 1:
                raise ValueError("iters must be an int32 device tensor")
            if each and (iters.numel() < B or not iters.is_contiguous()):
                raise ValueError("iters must be a contiguous int32 device tensor of at least B entries")
            it_ptr = iters.data_ptr()
        if each:
            _lib.check(_lib.load().ibl_float_decode_each(self._h, llr.data_ptr(), _DT_FL[llr.dtype], B,
                                                         out.data_ptr(), _DT_FL[out.dtype], it_ptr,
                                                         _stream_ptr(self.device)), "ibl_float_decode_each")
            return out
        _lib.check(_lib.load().ibl_float_decode(self._h, llr.data_ptr(), _DT_FL[llr.dtype], B, out.data_ptr(),
                                                _DT_FL[out.dtype], int(bool(early_stop)), it_ptr,
                                                _stream_ptr(self.device)), "ibl_float_decode")
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().ibl_float_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None


class LayeredDecoder:
    """Layered (row-serial) normalised / offset min-sum decoder, fp32 (``ibl_layered``; semantics in
    include/ibldpc.h "Layered min-sum"). ``layers``: ordered sequences of check indices (``codes.qc_layers``,
    ``codes.greedy_layers``). ``alpha`` scales and ``beta`` offsets the check magnitudes (1, 0: plain layered
    min-sum). The early stop is per codeword; ``decode(..., iters=)`` receives each codeword's iteration count.
    ``path``: ``"fused"`` (default) the on-chip kernel, one wave per codeword in LDS; ``"passes"`` per-layer
    kernels over HBM for codes of any length (``codes.dvbs2_layers`` for DVB-S2; they own about 4 N + 12 n_c
    bytes per codeword of ``max_batch``); ``"auto"`` the fused kernel when the codeword fits, else the per-layer
    kernels. The outputs are the same on every path.
    Check degrees 2..32: a code with a check of degree above 16 (DVB-S2 rates 4/5 to 9/10, 5G NR base graph 1)
    makes a *wide* decoder (:attr:`wide`), which runs kernels of its own on either path and keeps four state words
    per check instead of three (4 N + 16 n_c bytes per codeword, in LDS for the fused fit as in HBM). Every other
    decoder is what it was.
    ``compact`` (per-layer kernels only): ``True`` or ``(every, min_free_pct)`` moves the running codewords together
    between iterations so that whole tiles of finished ones are skipped (``ibl_layered_set_compaction``; the policy
    is in include/ibldpc.h). Values and iteration counts do not change; ``out`` may be written before the decode's
    last kernel. ``True`` means ``COMPACT_DEFAULT``.
    Raises :class:`_lib.IBLError` (``IBL_EUNSUPPORTED``) when ``path="fused"`` and a codeword does not fit in
    LDS, ``precision`` is not float32, or ``compact`` is given and the fused kernel is in use."""

    _PATHS = {"auto": _lib.IBL_PATH_AUTO, "passes": _lib.IBL_PATH_PASSES, "fused": _lib.IBL_PATH_FUSED}
    COMPACT_DEFAULT = (2, 25)   # the best measured pair: DESIGN.md "Layered min-sum: compaction"

    def __init__(self, graph: Graph, layers, imax: int, max_batch: int, alpha: float = 1.0, beta: float = 0.0,
                 llr_max: float = 150.0, precision=torch.float32, path: str = "fused", compact=None):
        if path not in self._PATHS:
            raise ValueError('path must be "fused", "passes" or "auto"')
        self.path = path
        self.graph = graph
        self.imax = int(imax)
        self.max_batch = int(max_batch)
        self.alpha, self.beta, self.llr_max = float(alpha), float(beta), float(llr_max)
        self.device = graph.device
        if precision not in _DT_FL:
            raise ValueError("precision must be torch.float32 (float64 is refused by the library)")
        nl, ptr, chk = _lib.pack_layers(layers)
        if chk.size == 0:
            chk = np.zeros(1, np.int32)
        self.n_layers = nl
        h = ctypes.c_void_p()
        _lib.check(_lib.load().ibl_layered_create_path(graph.handle, nl, ptr, chk, self.imax, self.alpha, self.beta,
                                                       self.llr_max, _DT_FL[precision], self.max_batch,
                                                       self._PATHS[path], ctypes.byref(h)),
                   "ibl_layered_create_path")
        self._h = h
        self._compaction = None
        if compact is not None and compact is not False:
            self.compaction = compact

    @property
    def compaction(self):
        """``None`` (off) or ``(every, min_free_pct)``. Assigning ``True``, a pair, or ``None`` / ``False``
        switches it for the decodes that follow (``ibl_layered_set_compaction``)."""
        return self._compaction

    @compaction.setter
    def compaction(self, value):
        if value is None or value is False:
            pair = None
        elif value is True:
            pair = self.COMPACT_DEFAULT
        else:
            every, pct = value
            pair = (int(every), int(pct))
            if pair != (every, pct):
                raise ValueError("compact must be True or a pair of integers (every, min_free_pct)")
            if pair[0] < 1:
                raise ValueError("compact: every must be >= 1 (None switches compaction off)")
        every, pct = pair if pair else (0, 0)
        _lib.check(_lib.load().ibl_layered_set_compaction(self._h, every, pct), "ibl_layered_set_compaction")
        self._compaction = pair

    def compaction_stats(self, stream=None):
        """``(compactions, extent)`` of the last decode: how often the running codewords were moved together and
        the columns in use at its end (``(0, B)`` without compaction). A diagnostic read-back: it waits for
        ``stream`` (default: the current stream of the decoder's device), which must be the decode's."""
        ptr = _stream_ptr(self.device) if stream is None else stream.cuda_stream
        n, e = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().ibl_layered_compaction_stats(self._h, ptr, ctypes.byref(n), ctypes.byref(e)),
                   "ibl_layered_compaction_stats")
        return int(n.value), int(e.value)

    @property
    def wide(self) -> bool:
        """Whether the code has a check of degree above 16, so that decodes run the wide kernels and state layout
        (``ibl_layered_is_wide``)."""
        w = ctypes.c_int32()
        _lib.check(_lib.load().ibl_layered_is_wide(self._h, ctypes.byref(w)), "ibl_layered_is_wide")
        return bool(w.value)

    @property
    def path_in_use(self) -> str:
        """``"fused"`` or ``"passes"``: the kernels decodes run (``ibl_layered_path_in_use``)."""
        f = ctypes.c_int32()
        _lib.check(_lib.load().ibl_layered_path_in_use(self._h, ctypes.byref(f)), "ibl_layered_path_in_use")
        return "fused" if f.value else "passes"

    def geometry(self, B: int):
        """``(cw_per_group, ngroups, grid)`` a batch of ``B`` is decoded with (``ibl_layered_geometry``): a
        workgroup decodes ``cw_per_group`` consecutive codewords at a time, workgroup w the groups w, w + grid, ...
        ``(0, 0, 0)`` on a per-layer decoder."""
        c, n, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().ibl_layered_geometry(self._h, int(B), ctypes.byref(c), ctypes.byref(n),
                                                    ctypes.byref(g)), "ibl_layered_geometry")
        return int(c.value), int(n.value), int(g.value)

    def decode(self, llr: torch.Tensor, out: Optional[torch.Tensor] = None, early_stop: bool = True,
               iters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``llr`` [N][B] float32 on the decoder's device -> APP LLRs [N][B] float32; ``iters``: int32 [B] device
        tensor receiving the iterations each codeword ran."""
        n = self.graph.edges.n_v
        _check_tensor(llr, self.device, n, "channel LLRs")
        if llr.dtype != torch.float32:
            raise ValueError("channel LLRs must be float32")
        B = llr.shape[1]
        if out is None:
            out = torch.empty((n, B), dtype=torch.float32, device=self.device)
        _check_tensor(out, self.device, n, "output")
        if out.dtype != torch.float32 or out.shape[1] != B:
            raise ValueError("output must be float32 [N][B]")
        it_ptr = None
        if iters is not None:
            if iters.dtype != torch.int32 or iters.device != self.device or iters.numel() < B \
                    or not iters.is_contiguous():
                raise ValueError("iters must be a contiguous int32 device tensor of at least B entries")
            it_ptr = iters.data_ptr()
        _lib.check(_lib.load().ibl_layered_decode(self._h, llr.data_ptr(), _lib.IBL_F32, B, out.data_ptr(),
                                                  _lib.IBL_F32, int(bool(early_stop)), it_ptr,
                                                  _stream_ptr(self.device)), "ibl_layered_decode")
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().ibl_layered_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None


class LayeredBPDecoder:
    """Layered (row-serial) belief-propagation decoder (``ibl_layered_create_bp``; semantics in
    include/ibldpc.h "Layered BP"): the schedule, layers and per-codeword early stop of :class:`LayeredDecoder`
    with the box-plus check update of the flooding fp32 BP decoder. ``path``: ``"fused"`` (default) the on-chip
    kernel, one wave per codeword with its APP values and one fp32 message per edge in LDS (4 N + 4 E bytes a
    codeword, up to 8 codewords a workgroup); ``"passes"`` per-layer kernels over HBM for codes of any length
    (``codes.dvbs2_layers`` for DVB-S2; about 4 N + 4 E bytes per codeword of ``max_batch``: 1.17 MB for DVB-S2
    rate 1/2); ``"auto"`` the fused kernel when the codeword fits. Both paths give the same bits.
    ``state_dtype``: ``torch.float32`` (default) or ``torch.float16``. With float16 the APP values and the messages
    are stored as IEEE binary16 while every operation stays fp32 (``ibl_layered_create_bp_half``; include/ibldpc.h
    "Layered BP, half-precision state"): 2 N + 2 E bytes a codeword on either path, so a code of twice the size fits
    the fused kernel and an iteration of the per-layer kernels moves half the bytes. Input and output stay float32
    (every output value is a binary16 value); meaningful decoding needs ``|llr| + 16 llr_max <= 65504``.
    :attr:`half` tells which state a decoder keeps.
    Check degrees 2..16. Raises :class:`_lib.IBLError` (``IBL_EUNSUPPORTED``) for a check above degree 16 and when
    ``path="fused"`` and a codeword does not fit in LDS. There is no compaction."""

    _PATHS = LayeredDecoder._PATHS
    _STATE = (torch.float32, torch.float16)

    def __init__(self, graph: Graph, layers, imax: int, max_batch: int, llr_max: float = 150.0, path: str = "fused",
                 precision=torch.float32, state_dtype=torch.float32):
        if path not in self._PATHS:
            raise ValueError('path must be "fused", "passes" or "auto"')
        if state_dtype not in self._STATE:
            raise ValueError("state_dtype must be torch.float32 or torch.float16")
        self.path = path
        self.state_dtype = state_dtype
        self.graph = graph
        self.imax = int(imax)
        self.max_batch = int(max_batch)
        self.llr_max = float(llr_max)
        self.device = graph.device
        if precision not in _DT_FL:
            raise ValueError("precision must be torch.float32 (float64 is refused by the library)")
        nl, ptr, chk = _lib.pack_layers(layers)
        if chk.size == 0:
            chk = np.zeros(1, np.int32)
        self.n_layers = nl
        h = ctypes.c_void_p()
        if state_dtype == torch.float16:
            if precision != torch.float32:
                raise ValueError("state_dtype=torch.float16 computes in float32: precision must be torch.float32")
            _lib.check(_lib.load().ibl_layered_create_bp_half(graph.handle, nl, ptr, chk, self.imax, self.llr_max,
                                                              self.max_batch, self._PATHS[path], ctypes.byref(h)),
                       "ibl_layered_create_bp_half")
        else:
            _lib.check(_lib.load().ibl_layered_create_bp(graph.handle, nl, ptr, chk, self.imax, self.llr_max,
                                                         _DT_FL[precision], self.max_batch, self._PATHS[path],
                                                         ctypes.byref(h)), "ibl_layered_create_bp")
        self._h = h

    @property
    def half(self) -> bool:
        """Whether the decoder keeps its state in binary16 (``ibl_layered_is_half``)."""
        w = ctypes.c_int32()
        _lib.check(_lib.load().ibl_layered_is_half(self._h, ctypes.byref(w)), "ibl_layered_is_half")
        return bool(w.value)

    path_in_use = LayeredDecoder.path_in_use
    geometry = LayeredDecoder.geometry
    decode = LayeredDecoder.decode
    __del__ = LayeredDecoder.__del__


class LayeredFixedDecoder:
    """Layered min-sum in fixed point (``ibl_layered_create_fixed``; semantics in include/ibldpc.h "Layered
    min-sum, fixed point"): 8-bit APP values, messages saturated at ``q_max``, magnitudes corrected as
    ``max(((alpha16 * m + 8) >> 4) - beta_q, 0)``, float LLRs quantised as ``rint(llr * scale)``. It runs the
    per-layer kernels over HBM (``path`` ``"auto"`` or ``"passes"``; ``"fused"`` raises :class:`_lib.IBLError`,
    ``IBL_EUNSUPPORTED``: that kernel is not built) and owns about N + 4 n_c + N / 8 bytes per codeword of
    ``max_batch``. ``decode`` takes and gives float32 or int8 tensors in any combination.
    ``path="onchip"`` runs the fused on-chip kernel of the same arithmetic instead
    (``ibl_layered_create_fixed_fused``): one wave per codeword in LDS, three launches per decode, the same values
    and iteration counts. A codeword needs N (rounded up to 4) + 4 n_c bytes of LDS, a workgroup holds up to 4;
    a code that does not fit (DVB-S2 N = 64800) raises ``IBL_EUNSUPPORTED``. :attr:`path_in_use` is then
    ``"fused"`` and :meth:`geometry` the real one. ``"auto"`` never chooses it.
    Check degrees 2..32: a code with a check of degree above 16 makes a *wide* decoder (:attr:`wide`) with two state
    words per check and codeword, N + 8 n_c + N / 8 bytes per codeword (on chip: N + 8 n_c of LDS)."""

    _PATHS = {**LayeredDecoder._PATHS, "onchip": None}   # "onchip" is an entry point of its own, not a path value
    _DT = {torch.float32: _lib.IBL_F32, torch.int8: _lib.IBL_I8}

    def __init__(self, graph: Graph, layers, imax: int, max_batch: int, alpha16: int = 16, beta_q: int = 0,
                 q_max: int = 31, scale: float = 2.0, path: str = "auto"):
        if path not in self._PATHS:
            raise ValueError('path must be "fused", "passes", "auto" or "onchip"')
        self.path = path
        self.graph = graph
        self.imax = int(imax)
        self.max_batch = int(max_batch)
        self.alpha16, self.beta_q, self.q_max, self.scale = int(alpha16), int(beta_q), int(q_max), float(scale)
        self.device = graph.device
        nl, ptr, chk = _lib.pack_layers(layers)
        if chk.size == 0:
            chk = np.zeros(1, np.int32)
        self.n_layers = nl
        h = ctypes.c_void_p()
        if path == "onchip":
            _lib.check(_lib.load().ibl_layered_create_fixed_fused(graph.handle, nl, ptr, chk, self.imax, self.alpha16,
                                                                  self.beta_q, self.q_max, self.scale, self.max_batch,
                                                                  ctypes.byref(h)),
                       "ibl_layered_create_fixed_fused")
        else:
            _lib.check(_lib.load().ibl_layered_create_fixed(graph.handle, nl, ptr, chk, self.imax, self.alpha16,
                                                            self.beta_q, self.q_max, self.scale, self.max_batch,
                                                            self._PATHS[path], ctypes.byref(h)),
                       "ibl_layered_create_fixed")
        self._h = h

    path_in_use = LayeredDecoder.path_in_use
    wide = LayeredDecoder.wide
    geometry = LayeredDecoder.geometry
    __del__ = LayeredDecoder.__del__

    def decode(self, llr: torch.Tensor, out: Optional[torch.Tensor] = None, out_dtype=None,
               early_stop: bool = True, iters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``llr`` [N][B] float32 (quantised with ``scale``) or int8 (integer units) on the decoder's device -> APP
        values [N][B] of ``out_dtype`` (default: ``out``'s, else ``llr``'s): int8 integer units, or float32 divided
        by ``scale``. ``out`` may be ``llr`` when the dtypes match. ``iters`` as :meth:`LayeredDecoder.decode`."""
        n = self.graph.edges.n_v
        _check_tensor(llr, self.device, n, "channel LLRs")
        if llr.dtype not in self._DT:
            raise ValueError("channel LLRs must be float32 or int8")
        B = llr.shape[1]
        if out_dtype is None:
            out_dtype = llr.dtype if out is None else out.dtype
        if out_dtype not in self._DT:
            raise ValueError("out_dtype must be torch.float32 or torch.int8")
        if out is None:
            out = torch.empty((n, B), dtype=out_dtype, device=self.device)
        _check_tensor(out, self.device, n, "output")
        if out.dtype != out_dtype or out.shape[1] != B:
            raise ValueError("output must be [N][B] of out_dtype")
        it_ptr = None
        if iters is not None:
            if iters.dtype != torch.int32 or iters.device != self.device or iters.numel() < B \
                    or not iters.is_contiguous():
                raise ValueError("iters must be a contiguous int32 device tensor of at least B entries")
            it_ptr = iters.data_ptr()
        _lib.check(_lib.load().ibl_layered_decode(self._h, llr.data_ptr(), self._DT[llr.dtype], B, out.data_ptr(),
                                                  self._DT[out_dtype], int(bool(early_stop)), it_ptr,
                                                  _stream_ptr(self.device)), "ibl_layered_decode")
        return out


def count_below(x: torch.Tensor, rows: int, threshold: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device count of ``x[:rows] < threshold`` (the reference's error counters) -> int64 tensor."""
    if x.dim() != 2 or not x.is_contiguous() or x.device.type != "cuda":
        raise ValueError("x must be a contiguous 2-D device tensor")
    if x.dtype not in _DT_ANY:
        raise ValueError("unsupported dtype")
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=x.device)
    rows = min(int(rows), x.shape[0])
    _lib.check(_lib.load().ibl_count_below(x.data_ptr(), _DT_ANY[x.dtype], rows, x.shape[1], x.shape[1],
                                           float(threshold), out.data_ptr(), _stream_ptr(x.device)),
               "ibl_count_below")
    return out


def philox_blocks(n: int, B: int) -> int:
    """Philox counter blocks one channel batch of n*B values consumes (4 values per block)."""
    return (int(n) * int(B) + 3) // 4


def channel_sample(out: torch.Tensor, cdf: np.ndarray, seed: int, offset: int,
                   llr: Optional[np.ndarray] = None, bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Direct-inversion channel samples on the device (``ibl_channel_sample``; the reference's
    ``quantize_direct_OpenCL`` / ``quantize_direct_OpenCL_LLR``, AWGN_Quantizer_BPSK.py:216-260).

    ``out``: contiguous [n][B] device tensor — uint8 / int32 receive cluster ids, float32 / float64
    receive ``llr[cluster]``. ``cdf``: the quantiser's T+1 CDF of p(t | x = 0). Uniforms come from
    numpy-compatible Philox4x64-10 (counter ``offset``, key ``seed``); the batch consumes
    :func:`philox_blocks` counter blocks. ``bits`` (optional [n][B] uint8 device tensor): codeword
    bits, 1 mirrors the cluster."""
    if out.dim() != 2 or not out.is_contiguous() or out.device.type != "cuda":
        raise ValueError("out must be a contiguous 2-D device tensor")
    if out.dtype not in _DT_ANY:
        raise ValueError("out dtype must be uint8, int32, float32 or float64")
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    T = len(cdf) - 1
    llr_arr = None
    if out.dtype in _DT_FL:
        if llr is None or len(llr) != T:
            raise ValueError("LLR output needs llr with T entries")
        llr_arr = np.ascontiguousarray(llr, dtype=np.float64)
    n, B = out.shape
    bptr = None
    if bits is not None:
        if bits.dtype != torch.uint8 or bits.shape != out.shape or not bits.is_contiguous() or bits.device != out.device:
            raise ValueError("bits must be a contiguous uint8 tensor shaped like out, on the same device")
        bptr = bits.data_ptr()
    _lib.check(_lib.load().ibl_channel_sample(cdf, T, None if llr_arr is None else llr_arr.ctypes.data,
                                              int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), n, B, bptr,
                                              out.data_ptr(), _DT_ANY[out.dtype], B, _stream_ptr(out.device)),
               "ibl_channel_sample")
    return out


class Encoder:
    """Batched systematic LDPC encoder on one device (``ibl_encoder``; the reference's
    Discrete_LDPC_decoding/LDPC_encoder.py plan :197-269 and encode :86-123, for B words at once)."""

    def __init__(self, H, max_batch: int, device=None):
        from .codes import canonical_csr
        self.device = _require_gpu(device)
        Hc = canonical_csr(H)
        self.N_c, self.N = Hc.shape
        self.K = self.N - self.N_c
        self.max_batch = int(max_batch)
        h = ctypes.c_void_p()
        _lib.check(_lib.load().ibl_encoder_create(self.N, self.N_c, np.ascontiguousarray(Hc.indptr, np.int32),
                                                  np.ascontiguousarray(Hc.indices, np.int32), self.max_batch,
                                                  self.device.index, ctypes.byref(h)), "ibl_encoder_create")
        self._h = h
        self.algorithm = _lib.load().ibl_encoder_algorithm(h).decode()

    def encode(self, info: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """u8 [K][B] information bits on the device -> u8 [N][B] codewords [info; parity]."""
        _check_tensor(info, self.device, self.K, "info")
        if info.dtype != torch.uint8:
            raise ValueError("info must be uint8")
        B = info.shape[1]
        if out is None:
            out = torch.empty((self.N, B), dtype=torch.uint8, device=self.device)
        _check_tensor(out, self.device, self.N, "out")
        if out.dtype != torch.uint8 or out.shape[1] != B:
            raise ValueError("out must be a uint8 [N][B] tensor")
        _lib.check(_lib.load().ibl_encode(self._h, info.data_ptr(), B, out.data_ptr(), _stream_ptr(self.device)),
                   "ibl_encode")
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().ibl_encoder_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None


def random_bits(out: torch.Tensor, seed: int, offset: int) -> torch.Tensor:
    """Fill a contiguous u8 [n][B] device tensor with information bits from the numpy-compatible
    Philox4x64-10 stream (top bit of each output; consumes :func:`philox_blocks` counter blocks)."""
    if out.dim() != 2 or not out.is_contiguous() or out.device.type != "cuda" or out.dtype != torch.uint8:
        raise ValueError("out must be a contiguous 2-D uint8 device tensor")
    n, B = out.shape
    _lib.check(_lib.load().ibl_random_bits(int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), n, B,
                                           out.data_ptr(), _stream_ptr(out.device)), "ibl_random_bits")
    return out


def count_errors(x: torch.Tensor, rows: int, threshold: float, bits: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device count of decided bits ``x[:rows] < threshold`` that differ from ``bits[:rows]`` -> int64."""
    if x.dim() != 2 or not x.is_contiguous() or x.device.type != "cuda" or x.dtype not in _DT_ANY:
        raise ValueError("x must be a contiguous 2-D device tensor (uint8/int32/float32/float64)")
    if bits.dtype != torch.uint8 or bits.dim() != 2 or not bits.is_contiguous() or bits.device != x.device \
            or bits.shape[1] != x.shape[1]:
        raise ValueError("bits must be a contiguous uint8 [n][B] tensor on x's device")
    rows = min(int(rows), x.shape[0], bits.shape[0])
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=x.device)
    _lib.check(_lib.load().ibl_count_errors(x.data_ptr(), _DT_ANY[x.dtype], rows, x.shape[1], x.shape[1],
                                            float(threshold), bits.data_ptr(), bits.shape[1], out.data_ptr(),
                                            _stream_ptr(x.device)), "ibl_count_errors")
    return out
