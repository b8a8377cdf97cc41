"""MI355X-native batched LDPC decoding (information-bottleneck LUT, min-sum, belief propagation).

Drop-in for the decoder classes of mx-strk/InformationBottleneckDecodingLDPC:

    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder_irreg import \
        Discrete_LDPC_Decoder_class_irregular
    from informationbottleneckdecodingldpc_amd.discrete_LDPC_decoder import Discrete_LDPC_Decoder_class
    from informationbottleneckdecodingldpc_amd.min_sum_decoder_irreg import Min_Sum_Decoder_class_irregular
    from informationbottleneckdecodingldpc_amd.bp_decoder_irreg import BeliefPropagationDecoderClassIrregular

plus a layered normalised / offset min-sum decoder the reference does not have:

    from informationbottleneckdecodingldpc_amd import Min_Sum_Layered_Decoder_class_irregular

and its belief-propagation counterpart (box-plus check update on the same schedule):

    from informationbottleneckdecodingldpc_amd import BeliefPropagation_Layered_Decoder_class_irregular

and for the channel side / drivers:

    from informationbottleneckdecodingldpc_amd.awgn_quantizer import AWGN_Channel_Quantizer  # device sampling
    from informationbottleneckdecodingldpc_amd.ber import BERConfig, run_ber                 # Eb/N0 sweeps
    from informationbottleneckdecodingldpc_amd.tables_io import load_decoder_config          # .npz/.json/.pkl

Decoding runs only in the hand-written HIP kernels of ``libibldpc.so`` (gfx950); see DESIGN.md.
"""
from . import codes, graph, tables, tables_io  # noqa: F401  (host-side set-up, importable without a GPU)

__version__ = "0.2.0"


def __getattr__(name):
    # the layered min-sum class (no reference counterpart); imported on first use: it needs torch
    if name == "Min_Sum_Layered_Decoder_class_irregular":
        from .min_sum_layered_decoder_irreg import Min_Sum_Layered_Decoder_class_irregular
        return Min_Sum_Layered_Decoder_class_irregular
    if name == "BeliefPropagation_Layered_Decoder_class_irregular":
        from .bp_layered_decoder_irreg import BeliefPropagation_Layered_Decoder_class_irregular
        return BeliefPropagation_Layered_Decoder_class_irregular
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def library_path() -> str:
    from ._lib import LIB_PATH
    return LIB_PATH
