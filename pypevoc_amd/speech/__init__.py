"""Drop-in for pypevoc/speech: the analysis functions, under both names the reference's package gives them
(pypevoc/speech/__init__.py:3: `analysis`), glottal inverse filtering, the formant tracker (`formants`: Formants, lpc,
lpc2form and lpcc2pole, which SpeechAnalysis and glottal keep as stubs) and its spectral-envelope half (`envelope`:
lpc2form_full and Formants(full=True)), the speech segmenter (`segmenter`: SpeechSegmenter, peaks,
refine_transition_points and the batched transition_points_rows; SEGMENT.md), the pitch-jump detector (`jumps`:
JumpDetector, zscore_wind, linreg_err, linreg2_err, the batched jumps_rows and segment_and_detect_jumps; JUMPS.md) and
the silence detector it segments with (`chunker`: SilenceDetector with the percentile discriminator, imported from that
module and not exported here) and the fricative descriptors (`fricatives`: FricativeDataFromSnip, the batched welch_rows,
fricative_desc_rows and fricative_rows, and fricative_intervals; FRICATIVES.md).  SyllableSegmenter and
MultiChannelSegmenter are not mirrored."""
from . import SpeechAnalysis  # noqa: F401
from . import glottal  # noqa: F401
from . import formants  # noqa: F401
from . import envelope  # noqa: F401
from . import segmenter  # noqa: F401
from . import jumps  # noqa: F401
from . import chunker  # noqa: F401
from . import fricatives  # noqa: F401
from .segmenter import SpeechSegmenter, peaks, refine_transition_points, transition_points_rows  # noqa: F401
from .jumps import JumpDetector  # noqa: F401

analysis = SpeechAnalysis
