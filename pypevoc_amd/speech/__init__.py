"""Drop-in for pypevoc/speech: the analysis functions, under both names the reference's package gives them
(pypevoc/speech/__init__.py:3: `analysis`), and glottal inverse filtering.  Its segmenter classes are not mirrored
(INTEGRATION.md)."""
from . import SpeechAnalysis  # noqa: F401
from . import glottal  # noqa: F401

analysis = SpeechAnalysis
