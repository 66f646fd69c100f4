"""MI355X-native sliding-window QLDPC decoder.

Host-side problem construction (codes, circuit, windows) is pure numpy/scipy and importable
anywhere; the decoder classes need libswd_hip.so and a gfx950 GPU and raise otherwise.
"""
from .decoders import (CircuitSampler, CodeCapacityExperiment, CodeCapacityResult, DemSampler, MeasurementFrontEnd, MeasurementSession, RollingMeasurementSession, MemoryExperiment, MemoryResult, PauliSampler, RollingDemSampler, RollingMemoryExperiment, RollingMemoryResult, RollingSession, SlidingWindowDecoder, SlidingWindowSession, SlidingWindowStream, bp4_osd, bp_history_decoder, bpgd_decoder,  # noqa: F401
                       bpgdg_decoder, group_account_device, osd_window, window_forms)
from ._lib import CapacityError  # noqa: F401
from .codes import CSSCode, create_surface_codes, hypergraph_product, rep_code  # noqa: F401
from .phenomenological import css_phenomenological_dem, phenomenological_dem  # noqa: F401
from .measurements import MeasurementMap, measurement_map, phenomenological_measurement_map  # noqa: F401

# The reference's classes imitate the `ldpc` v1 names (error text of osd_window.pyx:197, BASELINE north star):
# bp_decoder / bposd_decoder are the same objects under those spellings.  (The third-party ldpc.BpOsdDecoder of
# the harness's shorten=False branch is a different algorithm with no pinned version: not provided.)
bp_decoder = bp_history_decoder
bposd_decoder = osd_window

__all__ = ["osd_window", "bpgdg_decoder", "bpgd_decoder", "bp_history_decoder", "bp4_osd", "SlidingWindowDecoder",
           "SlidingWindowStream", "SlidingWindowSession", "RollingSession", "bp_decoder", "bposd_decoder", "DemSampler", "PauliSampler",
           "CodeCapacityExperiment", "CodeCapacityResult", "MemoryExperiment", "MemoryResult", "RollingDemSampler", "RollingMemoryExperiment",
           "RollingMemoryResult", "group_account_device", "window_forms", "CSSCode", "rep_code", "hypergraph_product", "create_surface_codes",
           "phenomenological_dem", "css_phenomenological_dem", "MeasurementFrontEnd", "MeasurementSession", "RollingMeasurementSession",
           "MeasurementMap", "measurement_map", "phenomenological_measurement_map", "CapacityError", "CircuitSampler"]
