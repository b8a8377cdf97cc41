"""Layered normalised / offset min-sum LDPC decoder with the interface of the float min-sum class
(:mod:`.min_sum_decoder_irreg`), running on the MI355X HIP kernels of ``ibl_layered_*``.

The reference has no layered decoder; this class keeps ``Min_Sum_Decoder_class_irregular``'s constructor shape
and method names so the same drivers (``ber.run_ber``) take it. Keyword-only extensions:

* ``layers`` — ordered sequences of check indices; or ``Z`` — the lifting size of a quasi-cyclic code, whose
  block rows become the layers (``codes.qc_layers``); neither: ``codes.greedy_layers``;
* ``alpha``, ``beta`` — normalisation factor and offset of the check magnitudes, max(alpha * m - beta, 0);
* ``path`` — ``"fused"`` (default), ``"passes"`` (per-layer kernels over HBM: long codes such as DVB-S2 with
  ``layers=codes.dvbs2_layers(H)``) or ``"auto"`` (:class:`.engine.LayeredDecoder`);
* ``fixed`` — ``True`` decodes in fixed point (:class:`.engine.LayeredFixedDecoder`, include/ibldpc.h "Layered
  min-sum, fixed point") with ``scale`` integer units per LLR unit and messages saturated at ``q_max``: ``alpha``
  must be a multiple of 1/16 in [0, 1] and ``beta * scale`` an integer in [0, 63]; ``llr_max`` is not used (the
  APP values saturate at 127 units); ``path`` ``"passes"`` or ``"auto"`` (``"fused"`` raises ``ValueError``), or
  ``"onchip"``: the fused on-chip kernel of the fixed-point arithmetic, for codes whose codeword fits the LDS
  (N + 4 n_c bytes; same results, ``ValueError`` without ``fixed=True`` or with ``compact``).
  Input and output stay float32;
* ``compact`` — ``True`` or ``(every, min_free_pct)``: the per-layer kernels move the running codewords together
  between iterations (:class:`.engine.LayeredDecoder`); same results. ``ValueError`` with ``fixed=True`` or
  ``path="fused"``.

Check degrees 2..32: a code with a check of degree above 16 (DVB-S2 rates 4/5 to 9/10) gets the engine's wide
kernels on every path and in either arithmetic, with nothing to ask for (:attr:`.engine.LayeredDecoder.wide`).

fp32 only unless ``fixed``. The early stop is per codeword; ``last_iterations`` holds the int32 device tensor of the last
decode's iteration counts.
"""
from __future__ import annotations

import numpy as np
import torch

from . import codes
from ._dropin import CodeMixin, resolve_device, to_device_input
from .engine import LayeredDecoder, LayeredFixedDecoder, count_below


class Min_Sum_Layered_Decoder_class_irregular(CodeMixin):

    _DECODER_NAME = "layered min-sum"   # in messages; the layered BP subclass names itself

    def __init__(self, filename, imax_, cardinality_T_channel_, msg_at_time_, *, layers=None, Z=None,
                 alpha: float = 1.0, beta: float = 0.0, llr_max: float = 150.0, path: str = "fused",
                 fixed: bool = False, scale: float = 2.0, q_max: int = 31, compact=None):
        if path not in LayeredFixedDecoder._PATHS:
            raise ValueError('path must be "fused", "passes" or "auto" (fixed=True: or "onchip")')
        self.path = path
        self.fixed = bool(fixed)
        if path == "onchip" and not self.fixed:
            raise ValueError('path="onchip" is the fixed-point fused kernel: it needs fixed=True (fp32: path="fused")')
        self.compact = None if compact is False else compact
        if self.compact is not None and (self.fixed or path == "fused"):
            raise ValueError('compact runs on the fp32 per-layer kernels: not with fixed=True or path="fused"')
        if self.fixed:
            if path == "fused":
                raise ValueError('fixed=True runs the per-layer kernels: path must be "passes" or "auto"')
            a16, bq = float(alpha) * 16.0, float(beta) * float(scale)
            if not (0.0 <= a16 <= 16.0 and a16 == int(a16)):
                raise ValueError("fixed=True: alpha must be a multiple of 1/16 in [0, 1]")
            if not (0.0 <= bq <= 63.0 and bq == int(bq)):
                raise ValueError("fixed=True: beta * scale must be an integer in [0, 63]")
            self.alpha16, self.beta_q, self.q_max, self.scale = int(a16), int(bq), int(q_max), float(scale)
        self._init_code(filename)
        self.imax = int(imax_)
        self.cardinality_T_channel = int(cardinality_T_channel_)
        self.set_code_parameters()
        self.data_len = int(self.R_c * self.codeword_len)
        self.msg_at_time = int(msg_at_time_)
        self.map_node_connections()
        if layers is not None and Z is not None:
            raise ValueError("give layers or Z, not both")
        if layers is None:
            layers = codes.qc_layers(self.H_sparse, Z) if Z is not None else codes.greedy_layers(self.H_sparse)
        self.layers = [np.asarray(l, dtype=np.int64) for l in layers]
        codes.validate_layers(self.H_sparse, self.layers)
        self.alpha, self.beta, self.llr_max = float(alpha), float(beta), float(llr_max)
        self.precision = torch.float32
        self.last_iterations = None
        self._dec = None
        self.device = None

    def init_OpenCL_decoding(self, msg_at_time_, context_=False):
        dev = resolve_device(context_)
        self.device = dev
        self.context = dev
        self.msg_at_time = int(msg_at_time_)
        if self.fixed:
            self._dec = LayeredFixedDecoder(self._graph_on(dev), self.layers, self.imax, self.msg_at_time,
                                            alpha16=self.alpha16, beta_q=self.beta_q, q_max=self.q_max,
                                            scale=self.scale, path=self.path)
            return
        self._dec = LayeredDecoder(self._graph_on(dev), self.layers, self.imax, self.msg_at_time, alpha=self.alpha,
                                   beta=self.beta, llr_max=self.llr_max, path=self.path,
                                   compact=self.compact)

    def _decode(self, received_blocks, buffer_in, return_buffer, early_stop=True):
        if self._dec is None:
            self.init_OpenCL_decoding(self.msg_at_time)
        llr = to_device_input(received_blocks, buffer_in, self.device, (torch.float32,))
        if llr.shape[1] > self._dec.max_batch:
            self.init_OpenCL_decoding(llr.shape[1], self.device)
        if not return_buffer and not bool(torch.isfinite(llr).all().item()):
            # host output synchronises anyway: the decoder's precondition is checked instead of returning
            # unspecified values
            raise ValueError(f"channel LLRs must be finite ({self._DECODER_NAME} precondition)")
        iters = torch.empty(llr.shape[1], dtype=torch.int32, device=self.device)
        out = self._dec.decode(llr, early_stop=early_stop, iters=iters)
        self.last_iterations = iters
        if return_buffer:
            return out
        return out.cpu().numpy()

    def decode_OpenCL_min_sum(self, received_blocks, buffer_in=False, return_buffer=False):
        return self._decode(received_blocks, buffer_in, return_buffer)

    def return_errors_all_zero(self, varnode_output_buffer):
        """Count of negative APP LLRs in the first data_len rows, as a float."""
        buf = varnode_output_buffer
        if not isinstance(buf, torch.Tensor):
            buf = torch.from_numpy(np.ascontiguousarray(buf, dtype=np.float32)).to(self.device)
        return float(count_below(buf.contiguous(), self.data_len, 0.0).item())
