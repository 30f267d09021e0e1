"""voicesplit_amd -- MI355X-native implementation of VoiceSplit's mask-prediction forward pass.

Public surface (mirrors the reference):

* ``VoiceSplit(config)`` / ``VoiceFilter(config)``: ``nn.Module`` classes with the reference's
  constructor, ``forward(x, speaker_embedding)`` signature and ``state_dict`` keys
  (models/voicesplit/model.py:9-89, models/voicefilter/model.py:11-90); also importable from the
  reference's own module paths ``models.voicesplit.model`` / ``models.voicefilter.model``.
* ``AttrDict`` / ``load_config``: the config object those constructors take
  (utils/generic_utils.py:560-573).
* ``SpeakerEncoder`` / ``logmel`` / ``mel_filterbank``: the GE2E speaker encoder that turns reference audio into the
  d-vector (notebooks/GE2E-Seungwonpark-ExtractSpeakerEmbedding-...py), ``voicesplit_amd/speaker.py``.
* ``resample.Resampler`` / ``resample.StreamingResampler`` / ``audio.resample``: sample-rate conversion on the device, the
  reference's ``librosa.load(path, sr=sample_rate)`` (``voicesplit_amd/resample.py``).
* ``loudness.LoudnessMeter`` / ``loudness.integrated_loudness`` / ``loudness.normalize``: ITU-R BS.1770-4 integrated loudness and a
  linear gain with a peak cap on the device, the loudness half of the reference's ``scripts/normalise-resample.sh``
  (``voicesplit_amd/loudness.py``; not ffmpeg's dynamic ``loudnorm``).
* ``metrics.bss_sdr`` / ``metrics.bss_eval`` / ``metrics.stoi``: the evaluation scores on the device: BSS-eval SDR, SIR, SAR and
  the intelligibility scores STOI / ESTOI (``voicesplit_amd/metrics.py``).
* ``ops``: stage-level entry points over the C ABI of ``libvoicesplit_hip.so``.

The compute path is the HIP library only; there is no PyTorch/CPU fallback.
"""
from .config import AttrDict, load_config, default_config  # noqa: F401
from .model import VoiceFilter, VoiceSplit  # noqa: F401
from .speaker import SpeakerEncoder, logmel, mel_filterbank  # noqa: F401

__all__ = ["VoiceSplit", "VoiceFilter", "AttrDict", "load_config", "default_config", "SpeakerEncoder", "logmel",
           "mel_filterbank"]
