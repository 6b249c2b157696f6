"""Drop-in for pypevoc/speech: the analysis functions, under both names the reference's package gives them
(pypevoc/speech/__init__.py:3: `analysis`), glottal inverse filtering, the formant tracker (`formants`: Formants, lpc,
lpc2form and lpcc2pole, which SpeechAnalysis and glottal keep as stubs) and its spectral-envelope half (`envelope`:
lpc2form_full and Formants(full=True)) and the speech segmenter (`segmenter`: SpeechSegmenter, peaks,
refine_transition_points and the batched transition_points_rows; SEGMENT.md).  SyllableSegmenter, SilenceDetector and
MultiChannelSegmenter are not mirrored."""
from . import SpeechAnalysis  # noqa: F401
from . import glottal  # noqa: F401
from . import formants  # noqa: F401
from . import envelope  # noqa: F401
from . import segmenter  # noqa: F401
from .segmenter import SpeechSegmenter, peaks, refine_transition_points, transition_points_rows  # noqa: F401

analysis = SpeechAnalysis
