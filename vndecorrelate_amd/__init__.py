"""vndecorrelate_amd - MI355X-native velvet-noise decorrelator.

Drop-in for the velvet-noise path of ckonst/VNDecorrelate: import
``vndecorrelate_amd.decorrelation`` where you imported
``vndecorrelate.decorrelation``.  The tap sum runs in hand-written HIP kernels
for gfx950 behind the C ABI of ``include/vnd_amd.h``; see DESIGN.md.
"""
__version__ = '0.1.0'

from .decorrelation import (  # noqa: F401
    MODE_EXACT,
    MODE_FAST,
    MODE_FMA,
    HaasEffect,
    SignalChain,
    VelvetNoise,
    WhiteNoise,
    convolve_velvet_noise,
    convolve_velvet_noise_bank,
    convolve_velvet_noise_batched,
    decorrelate_bank,
    decorrelate_each,
    decorrelate_each_stream,
    decorrelate_fade_voice_pool,
    decorrelate_voice_pool,
    each_covers,
    generate_velvet_noise,
    set_default_mode,
    set_device_epilogue,
    set_each_device,
    set_white_noise_device,
)
from .analysis import (  # noqa: F401
    CorrelogramVoicePool,
    LevelVoicePool,
    PolarVoicePool,
    ScopeVoicePool,
    correlogram_voice_spans,
    cross_correlogram_batched,
    cross_correlogram_voice_pool,
    lissajous_histogram_batched,
    lissajous_histogram_voice_pool,
    polar_coordinates_batched,
    polar_histogram_batched,
    polar_histogram_voice_pool,
    polar_level_batched,
    polar_level_voice_pool,
    polar_moments_ordered,
    polar_voice_spans,
    scope_covers,
    scope_voice_spans,
    scope_voice_window,
    set_correlogram_device,
    set_scope_device,
    stereo_image_voice_pool,
)
from .spectral import (  # noqa: F401
    SpectrumVoicePool,
    coherence_batched,
    csd_batched,
    set_spectrum_device,
    spectrogram_batched,
    spectrum_covers,
    spectrum_voice_pool,
    spectrum_voice_spans,
    welch_batched,
)
from .streaming import (  # noqa: F401
    ChainFadeVoicePool,
    ChainStream,
    ChainVoicePool,
    EachStream,
    FadeVoicePool,
    HaasEachStream,
    HaasFadeVoicePool,
    HaasStream,
    HaasVoicePool,
    Stream,
    VoicePool,
    convolve_velvet_noise_stream,
    fade_gains,
    haas_voice_fade_spans,
    haas_voice_spans,
    voice_fade_spans,
    voice_spans,
)
