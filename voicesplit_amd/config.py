"""Config object consumed by the model constructors.

Mirror of the reference's ``AttrDict`` / ``load_config`` (utils/generic_utils.py:560-573): a dict
whose keys are also attributes, read from JSON that may carry ``//`` comments.  Only what the hot
path's constructor reads is required: ``config.audio[config.audio['backend']]['num_freq']`` and
``config.model['emb_dim'|'lstm_dim'|'fc1_dim'|'fc2_dim']`` (models/voicesplit/model.py:13,57-64).
"""
import json
import re


class AttrDict(dict):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


def load_config(config_path: str) -> AttrDict:
    with open(config_path, "r") as fh:
        text = fh.read()
    text = re.sub(r"\\\n", "", text)
    text = re.sub(r"//.*\n", "\n", text)
    cfg = AttrDict()
    cfg.update(json.loads(text))
    return cfg


def default_config(num_freq: int = 601, emb_dim: int = 256, lstm_dim: int = 400,
                   fc1_dim: int = 600, fc2_dim: int = 601, model_name: str = "voicesplit") -> AttrDict:
    """The hot-path subset of the reference's config.json: model (lines 2, 37-42), the 'voicefilter'
    audio backend (44, 83-95; power and griffin_lim_iters feed audio.griffin_lim), the loss (16-20) and the training hyper-parameters (21-32; batch_size
    is the reference's 2 -- BASELINE's B=64 is set by the caller)."""
    cfg = AttrDict()
    cfg.update({
        "model_name": model_name,
        "model": {"lstm_dim": lstm_dim, "fc1_dim": fc1_dim, "fc2_dim": fc2_dim, "emb_dim": emb_dim},
        "audio": {"backend": "voicefilter", "audio_len": 3,
                  "voicefilter": {"n_fft": 2 * (num_freq - 1), "num_freq": num_freq, "sample_rate": 16000,
                                  "hop_length": 160, "win_length": 400, "min_level_db": -100.0, "ref_level_db": 20.0,
                                  "power": 1.5, "griffin_lim_iters": 60}},
        "loss": {"loss_name": "si_snr" if model_name == "voicesplit" else "power_law_compression",
                 "power": 0.30, "complex_loss_ratio": 0.113},
        "train_config": AttrDict({"epochs": 1000, "learning_rate": 1e-2, "optimizer": "adam", "batch_size": 2, "seed": 42,
                                  "num_workers": 14, "logs_path": "../checkpoints/", "reinit_layers": None,
                                  "summary_interval": 2, "checkpoint_interval": 500}),
    })
    return cfg


def reference_audio_blocks() -> dict:
    """The 'waveglow' and 'wavernn' blocks of the reference's config.json (lines 47-82), as ``config.audio`` carries them beside
    'voicefilter'.  ``default_config`` does not include them; put one into ``cfg.audio`` and set ``cfg.audio['backend']``."""
    return {
        "waveglow": {"segment_length": 16000, "sample_rate": 22050, "filter_length": 1024, "num_freq": 513, "n_mel_channels": 80,
                     "hop_length": 256, "win_length": 1024, "mel_fmin": 0.0, "mel_fmax": 8000.0, "power": 1.5,
                     "griffin_lim_iters": 60},
        "wavernn": {"force_convert_SR": True, "num_mels": 80, "num_freq": 1025, "sample_rate": 16000, "frame_length_ms": 50,
                    "frame_shift_ms": 12.5, "preemphasis": 0.98, "min_level_db": -100, "ref_level_db": 20, "signal_norm": True,
                    "symmetric_norm": False, "max_norm": 1, "clip_norm": True, "mel_fmin": 0.0, "mel_fmax": 8000.0,
                    "do_trim_silence": True, "power": 1.5, "griffin_lim_iters": 60},
    }


BACKENDS = ("voicefilter", "wavernn", "waveglow")


def audio_backend(block) -> str:
    """Which processor a block of ``config.audio`` belongs to, from its own keys (or its 'backend' entry once resolved)."""
    if "codec" in block and "backend" in block:
        return block["backend"]
    if "filter_length" in block:
        return "waveglow"
    if "frame_shift_ms" in block:
        return "wavernn"
    return "voicefilter"


def resolve_audio(cfg):
    """``config.audio`` (the whole section, with 'backend') or one of its blocks -> an audio block with the voicefilter-style keys
    every entry point reads: n_fft, hop_length, win_length, sample_rate, power, griffin_lim_iters, num_freq, plus 'backend',
    'codec' (how a linear magnitude is stored: csrc/audio_codec.hip), the mel settings ('num_mels', 'mel_fmin', 'mel_fmax') and
    'mel_spec'.  A voicefilter block comes back as it is (the same object); a resolved block likewise (idempotent).

    waveglow (WaveGlowAudioProcessor, utils/audio_processor.py:338-438): n_fft = filter_length, LOG codec, zero padding inside
    Griffin-Lim.  wavernn (WaveRNNAudioProcessor :61-336): n_fft = (num_freq - 1) * 2, hop / win = int(ms / 1000.0 * sample_rate)
    (:175-182), DBNORM codec, pre-emphasis."""
    import math
    mel_spec = None
    if "backend" in cfg and "codec" not in cfg:      # the whole section (a resolved block names its back end too, beside its codec)
        name = cfg["backend"]
        if name not in BACKENDS or not isinstance(cfg.get(name), dict):
            raise ValueError(f"Invalid AudioProcessor Backend: {name!r} (one of {BACKENDS}, with its block in config.audio)")
        mel_spec = cfg.get("mel_spec")
        block = cfg[name]
        if name == "voicefilter":
            return block
        found = audio_backend(block)
        if "codec" not in block and found != name:
            raise ValueError(f"config.audio['backend'] is {name!r} but its block has the keys of {found!r}")
    else:
        block, name = cfg, audio_backend(cfg)
    if "codec" in block or name == "voicefilter":
        return block
    out = AttrDict(block)
    sr = int(block["sample_rate"])
    if name == "waveglow":
        n_fft = int(block["filter_length"])
        if "num_freq" in block and int(block["num_freq"]) != n_fft // 2 + 1:
            raise ValueError(f"waveglow: num_freq {block['num_freq']} is not filter_length // 2 + 1 = {n_fft // 2 + 1}")
        out.update(n_fft=n_fft, num_freq=n_fft // 2 + 1, hop_length=int(block["hop_length"]), win_length=int(block["win_length"]),
                   num_mels=int(block.get("n_mel_channels", 80)))
        codec = {"kind": "LOG", "floor": 1e-5, "min_level_db": -100.0, "ref_level_db": 20.0, "signal_norm": False,
                 "symmetric_norm": False, "clip_norm": False, "max_norm": 1.0, "preemphasis": 0.0, "gl_pad": "zero"}
    else:
        n_fft = (int(block["num_freq"]) - 1) * 2
        min_db = float(block["min_level_db"])
        max_norm = block.get("max_norm")
        out.update(n_fft=n_fft, hop_length=int(block["frame_shift_ms"] / 1000.0 * sr), win_length=int(block["frame_length_ms"] / 1000.0 * sr),
                   num_mels=int(block.get("num_mels", 80)))
        codec = {"kind": "DBNORM", "floor": math.exp(min_db / 20 * math.log(10)), "min_level_db": min_db,
                 "ref_level_db": float(block["ref_level_db"]), "signal_norm": bool(block.get("signal_norm")),
                 "symmetric_norm": bool(block.get("symmetric_norm")), "clip_norm": bool(block.get("clip_norm", True)),
                 "max_norm": 1.0 if max_norm is None else float(max_norm), "preemphasis": float(block.get("preemphasis") or 0.0),
                 "gl_pad": "reflect"}
    fmin, fmax = block.get("mel_fmin"), block.get("mel_fmax")
    if fmax is not None and fmax > sr // 2:
        raise ValueError(f"{name}: mel_fmax {fmax} is above sample_rate // 2 = {sr // 2}")
    out.update(backend=name, sample_rate=sr, codec=codec, mel_fmin=0.0 if fmin is None else float(fmin),
               mel_fmax=None if fmax is None else float(fmax),
               mel_spec=bool(block.get("mel_spec", False) if mel_spec is None else mel_spec))
    return out
