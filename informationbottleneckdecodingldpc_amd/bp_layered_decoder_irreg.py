"""Layered belief-propagation LDPC decoder with the interface of the float BP class (:mod:`.bp_decoder_irreg`),
running on the MI355X HIP kernels of ``ibl_layered_create_bp`` (include/ibldpc.h "Layered BP").

The reference has no layered decoder. This class subclasses the layered min-sum class
(:mod:`.min_sum_layered_decoder_irreg`) the way the flooding BP class subclasses the flooding min-sum one: the same
constructor shape, ``decode_OpenCL_belief_propagation`` instead of ``decode_OpenCL_min_sum``, so ``ber.run_ber``
takes it as a BP decoder. Keyword-only extensions: ``layers``, ``Z`` and ``path`` (``"fused"``, ``"passes"``,
``"auto"``) as the min-sum class has them, ``llr_max``, and ``state_dtype`` (``torch.float32``, the default, or
``torch.float16``: the state kept in binary16, :class:`.engine.LayeredBPDecoder`). BP has no correction, fixed-point
form or compaction: ``alpha``, ``beta``, ``fixed`` and ``compact`` raise ``ValueError``.

fp32 arithmetic, input and output, check degrees 2..16. The early stop is per codeword; ``last_iterations`` holds the
int32 device tensor of the last decode's iteration counts.
"""
from __future__ import annotations

import torch

from .engine import LayeredBPDecoder
from .min_sum_layered_decoder_irreg import Min_Sum_Layered_Decoder_class_irregular
from ._dropin import resolve_device


class BeliefPropagation_Layered_Decoder_class_irregular(Min_Sum_Layered_Decoder_class_irregular):

    _DECODER_NAME = "layered BP"
    _REFUSED = ("alpha", "beta", "fixed", "compact")

    def __init__(self, filename, imax_, cardinality_T_channel_, msg_at_time_, *, layers=None, Z=None,
                 llr_max: float = 150.0, path: str = "fused", state_dtype=torch.float32, **refused):
        for name in refused:
            if name in self._REFUSED:
                raise ValueError(f"{name} is not a parameter of the layered BP decoder (no correction, fixed-point "
                                 "form or compaction is built for it)")
            raise TypeError(f"__init__() got an unexpected keyword argument {name!r}")
        if path not in LayeredBPDecoder._PATHS:
            raise ValueError('path must be "fused", "passes" or "auto"')
        if state_dtype not in LayeredBPDecoder._STATE:
            raise ValueError("state_dtype must be torch.float32 or torch.float16")
        self.state_dtype = state_dtype
        super().__init__(filename, imax_, cardinality_T_channel_, msg_at_time_, layers=layers, Z=Z, llr_max=llr_max,
                         path=path)

    def init_OpenCL_decoding(self, msg_at_time_, context_=False):
        dev = resolve_device(context_)
        self.device = dev
        self.context = dev
        self.msg_at_time = int(msg_at_time_)
        self._dec = LayeredBPDecoder(self._graph_on(dev), self.layers, self.imax, self.msg_at_time,
                                     llr_max=self.llr_max, path=self.path, state_dtype=self.state_dtype)

    def decode_OpenCL_belief_propagation(self, received_blocks, buffer_in=False, return_buffer=False):
        return self._decode(received_blocks, buffer_in, return_buffer)

    @property
    def decode_OpenCL_min_sum(self):
        """Not part of the BP class: reading the name raises, so ``hasattr`` is False."""
        raise AttributeError("BeliefPropagation_Layered_Decoder_class_irregular has no decode_OpenCL_min_sum")
