"""Waveforms -> the on-disk training format that data.py reads: the reference's preprocessing (src/preprocess.py:32-35
write_metadata, src/ljspeech.py:15-102 build_from_path / _process_utterance with input_type="raw") restated without its
absent dependencies (librosa, lws, nnmnkwii, TF-1 hparams).

Per utterance, as the reference: rescale to a peak of 0.999 (hparams_tacotron.py rescaling, rescaling_max); the mel
spectrogram (N, n_mels) float32 (audio.melspectrogram: one HIP kernel, the utterances sorted by length and sent in ragged
batches); the audio zero-padded by lws_pad_lr and cut to N * hop_size samples -- the reference pads the audio the way lws
would while it frames the mel with librosa; that mismatch is kept, it defines `timesteps`; `<name>-audio-%05d.npy`,
`<name>-mel-%05d.npy`, and one `train.txt` line `audio|mel|timesteps|text[|speaker]`.

Recordings at another rate, and silent ends (src/cmu_arctic.py:55-128, the multi-speaker writer): process_utterances(...,
resample=True, trim_top_db=20) reads each file at its own rate, resamples and trims on the device in ragged batches
(audio.resample, audio.trim_silence) and then runs the same rescale -> mel -> pad flow, in the reference's order: load and
resample, trim, rescale, mel.  build_from_path_cmu_arctic walks `cmu_us_<speaker>_arctic/wav/*.wav` and writes the speaker
id as the fifth field.  Both options are off by default, and then nothing differs from the LJSpeech path.

Not restated: the mu-law input types, the jsut / librivox walkers, the dead `.lab` branch of cmu_arctic.py (`and False`), a
process pool and the CLI.  parity unpinned, as for the rest of audio.py: tests hold the files to an fp64 restatement of the
formulas.
"""
from __future__ import annotations

import os
from os.path import join

import numpy as np
import torch

from . import audio

RESCALING_MAX = 0.999          # hparams_tacotron.py: rescaling = True, rescaling_max = 0.999


def lws_num_frames(length, fsize, fshift):
    """audio_tacotron.py:122-130: the number of frames lws would make of `length` samples."""
    pad = fsize - fshift
    if length % fshift == 0:
        return (length + pad * 2 - fsize) // fshift + 1
    return (length + pad * 2 - fsize) // fshift + 2


def lws_pad_lr(x, fsize, fshift):
    """audio_tacotron.py:133-140: the left and right zero padding lws applies internally."""
    M = lws_num_frames(len(x), fsize, fshift)
    pad = fsize - fshift
    T = len(x) + 2 * pad
    r = (M - 1) * fshift + fsize - T
    return pad, pad + r


TRIM_FRAME_LENGTH, TRIM_HOP_LENGTH = 2048, 512     # librosa.effects.trim's defaults, which cmu_arctic.py:72 leaves alone
# nnmnkwii.datasets.cmu_arctic.available_speakers as recalled (cmu_arctic.py:22); nnmnkwii is not here to check the list or
# its order, which fixes the speaker ids.
CMU_ARCTIC_SPEAKERS = ("awb", "bdl", "clb", "jmk", "ksp", "rms", "slt")


def _rescaled(label, wav, fft_size):
    if wav.ndim != 1 or len(wav) <= fft_size // 2:
        raise ValueError(f"{label}: {wav.shape} samples; need a 1-D clip longer than fft_size / 2 = {fft_size // 2}")
    peak = float(np.abs(wav).max())
    if not peak > 0.0 or not np.isfinite(peak):
        raise ValueError(f"{label}: an all-zero (or non-finite) clip cannot be rescaled")
    return (wav / peak * RESCALING_MAX).astype(np.float32)


def _resample_and_trim(wavs, rates, labels, sample_rate, trim_top_db, batch_clips, device):
    """The clips of `wavs` (each at its own rates[i]) at sample_rate, cut to audio.trim_silence's bounds when trim_top_db is
    set: grouped by rate, sorted by length, on the device in ragged batches of batch_clips, and back on the host.  The kernels
    give a clip what they give it alone, so the result does not depend on batch_clips."""
    shortest = TRIM_FRAME_LENGTH // 2 + 1 if trim_top_db is not None else 1
    for label, wav, sr in zip(labels, wavs, rates):
        P, Q = audio.resample_ratio(sr, sample_rate)
        if wav.ndim != 1 or -(-len(wav) * P // Q) < shortest:
            raise ValueError(f"{label}: {wav.shape} samples at {sr} Hz; need a 1-D clip of at least {shortest} samples at {sample_rate} Hz")
    out = [None] * len(wavs)
    for sr in sorted(set(rates)):
        order = sorted((i for i in range(len(wavs)) if rates[i] == sr), key=lambda i: len(wavs[i]))
        for s in range(0, len(order), batch_clips):
            idx = order[s:s + batch_clips]
            lens = np.array([len(wavs[i]) for i in idx], dtype=np.int32)
            batch = np.zeros((len(idx), int(lens.max())), dtype=np.float32)
            for r, i in enumerate(idx):
                batch[r, :lens[r]] = wavs[i]
            y, lens = audio.resample(torch.from_numpy(batch).to(device), sr, sample_rate, lengths=lens)
            bounds = np.stack([np.zeros_like(lens), lens], axis=1)
            if trim_top_db is not None:
                bounds = audio.trim_silence(y, trim_top_db, TRIM_FRAME_LENGTH, TRIM_HOP_LENGTH, lengths=lens).cpu().numpy()
            y = y.cpu().numpy()
            for r, i in enumerate(idx):
                out[i] = np.ascontiguousarray(y[r, bounds[r, 0]:bounds[r, 1]])
    return out


def _augmented(clips, labels, copies, seed, tempo_range, noise, noise_levels, sample_rate, batch_clips, device):
    """`copies` augmented versions of every clip, copy-major ([c * N + i] is copy c + 1 of clip i): a tempo change and, when noise
    is given, that recording mixed in (audio.tempo, audio.mix_noise at 0 dB gain).  Every parameter is drawn before anything
    runs, in that order, by audio.augment_draws from torch.Generator().manual_seed(seed) -- the gain is drawn too and not used,
    so the other values are the ones audio.random_augment would draw -- and the kernels give a clip what they give it alone: the
    result does not depend on batch_clips."""
    N = len(clips)
    if noise is not None:
        noise = audio.load_wav(noise, sample_rate) if isinstance(noise, (str, os.PathLike)) else np.ascontiguousarray(noise, dtype=np.float32)
        if noise.ndim != 1 or len(noise) < 1:
            raise ValueError(f"process_utterances: noise must be a 1-D recording, got {noise.shape}")
    params = audio.augment_draws(copies * N, torch.Generator().manual_seed(int(seed)), tempo_range, audio.GAIN_RANGE_DB,
                                 None if noise is None else len(noise), noise_levels)
    noise_d = None if noise is None else torch.from_numpy(noise).to(device)
    out = [None] * (copies * N)
    order = sorted(range(copies * N), key=lambda k: len(clips[k % N]))
    for s in range(0, len(order), batch_clips):
        idx = order[s:s + batch_clips]
        lens = np.array([len(clips[k % N]) for k in idx], dtype=np.int32)
        batch = np.zeros((len(idx), int(lens.max())), dtype=np.float32)
        for r, k in enumerate(idx):
            batch[r, :lens[r]] = clips[k % N]
        y, out_lens = audio.tempo(torch.from_numpy(batch).to(device), params["tempo"][idx], sample_rate, lengths=lens)
        if noise_d is not None:
            y = audio.mix_noise(y, noise_d, params["level"][idx], params["offset"][idx], lengths=out_lens)
        y = y.cpu().numpy()
        for r, k in enumerate(idx):
            out[k] = np.ascontiguousarray(y[r, :out_lens[r]])
    return out, ["%s (augmented copy %d)" % (labels[k % N], k // N + 1) for k in range(copies * N)]


def process_utterances(wavs, texts, out_dir, name="ljspeech", start_index=1, speaker_ids=None, sample_rate=22050, fft_size=1024,
                       hop_size=256, n_mels=80, batch_clips=64, device="cuda:0", resample=False, trim_top_db=None, augment_copies=0,
                       augment_seed=0, tempo_range=audio.TEMPO_RANGE, noise=None, noise_levels=audio.NOISE_LEVELS):
    """ljspeech._process_utterance over a list.  wavs: paths of PCM files (audio.load_wav) or 1-D float arrays; texts: one
    string each; speaker_ids: optional integers, appended as a fifth field.  Utterance i is written as
    `<name>-audio-%05d.npy` / `<name>-mel-%05d.npy` with number start_index + i.  Returns the metadata tuples
    (audio_filename, mel_filename, timesteps, text[, speaker]) in the order given.  The files do not depend on batch_clips.
    resample=True: a file at another rate is resampled to sample_rate instead of refused (arrays are taken to be at
    sample_rate).  trim_top_db: cut each clip to audio.trim_silence(clip, trim_top_db)'s span before the rescale, as
    cmu_arctic._process_utterance does with 20.  With both off (the default) every step is the LJSpeech path's.
    augment_copies = n > 0: every utterance is also written n times augmented, as the reference augments what it loads
    (util.py:122-134 and NoiseInjection): a tempo drawn from tempo_range and, when `noise` (a 1-D recording at sample_rate, or the
    path of one) is given, that recording mixed in from a random offset at a level drawn from noise_levels relative to the
    clip's RMS.  The augmentation runs after resample and trim and before the peak rescale; the reference's random gain is left
    out on purpose, because the rescale to a peak of 0.999 cancels it.  Copy c = 1 .. n of utterance i is number
    start_index + c * N + i (N utterances: the copies come after all the originals), with utterance i's text and speaker; the
    returned metadata is in number order, N * (1 + n) rows.  The originals' files are bit for bit what they are without
    augmentation.  All parameters are drawn up front from augment_seed (copy-major, then utterance order), so the files do not
    depend on batch_clips.  augment_copies = 0 (the default) is the path without augmentation."""
    if len(texts) != len(wavs) or (speaker_ids is not None and len(speaker_ids) != len(wavs)):
        raise ValueError("process_utterances: wavs, texts and speaker_ids must have one entry per utterance")
    if batch_clips < 1:
        raise ValueError("process_utterances: batch_clips must be at least 1")
    if trim_top_db is not None and not trim_top_db > 0:
        raise ValueError(f"process_utterances: trim_top_db must be positive or None, got {trim_top_db!r}")
    if isinstance(augment_copies, bool) or not isinstance(augment_copies, (int, np.integer)) or augment_copies < 0:
        raise ValueError(f"process_utterances: augment_copies must be a non-negative integer, got {augment_copies!r}")
    os.makedirs(out_dir, exist_ok=True)
    prepare = bool(resample) or trim_top_db is not None
    clips, rates, labels = [], [], []
    for i, w in enumerate(wavs):
        is_path = isinstance(w, (str, os.PathLike))
        label = str(w) if is_path else f"utterance {i}"
        if is_path and prepare:
            sr, wav = audio.read_wav(w)
            if sr != sample_rate and not resample:
                raise ValueError(f"{label}: sample rate {sr}, expected {sample_rate} (pass resample=True to resample it)")
        else:
            sr, wav = sample_rate, (audio.load_wav(w, sample_rate) if is_path else np.asarray(w, dtype=np.float32))
        clips.append(wav if prepare or augment_copies else _rescaled(label, wav, fft_size))
        rates.append(sr)
        labels.append(label)
    if prepare:
        clips = _resample_and_trim(clips, rates, labels, sample_rate, trim_top_db, batch_clips, device)
    n_utt = len(clips)
    if augment_copies:
        for label, wav in zip(labels, clips):
            if wav.ndim != 1 or len(wav) < 1:
                raise ValueError(f"{label}: {wav.shape} samples; need a 1-D clip that is not empty")
        more, more_labels = _augmented(clips, labels, int(augment_copies), augment_seed, tempo_range, noise, noise_levels, sample_rate,
                                       batch_clips, device)
        clips, labels = list(clips) + more, labels + more_labels
    if prepare or augment_copies:
        clips = [_rescaled(label, wav, fft_size) for label, wav in zip(labels, clips)]
    metadata = [None] * len(clips)
    order = sorted(range(len(clips)), key=lambda i: len(clips[i]))
    for s in range(0, len(order), batch_clips):
        idx = order[s:s + batch_clips]
        lens = np.array([len(clips[i]) for i in idx], dtype=np.int32)
        batch = np.zeros((len(idx), int(lens.max())), dtype=np.float32)
        for r, i in enumerate(idx):
            batch[r, :lens[r]] = clips[i]
        mels = audio.melspectrogram(torch.from_numpy(batch).to(device), sample_rate, fft_size, hop_size, n_mels, lengths=lens,
                                    layout="frame_major").cpu().numpy()
        for r, i in enumerate(idx):
            wav = clips[i]
            N = 1 + len(wav) // hop_size
            left, right = lws_pad_lr(wav, fft_size, hop_size)
            out = np.pad(wav, (left, right), mode="constant", constant_values=0.0)
            assert len(out) >= N * hop_size
            out = out[:N * hop_size]
            audio_filename, mel_filename = "%s-audio-%05d.npy" % (name, start_index + i), "%s-mel-%05d.npy" % (name, start_index + i)
            np.save(join(out_dir, audio_filename), out.astype(np.float32), allow_pickle=False)
            np.save(join(out_dir, mel_filename), np.ascontiguousarray(mels[r, :N]), allow_pickle=False)
            row = (audio_filename, mel_filename, len(out), texts[i % n_utt])
            metadata[i] = row + (int(speaker_ids[i % n_utt]),) if speaker_ids is not None else row
    return metadata


def write_metadata(metadata, out_dir):
    """preprocess.py:32-35: train.txt, one line per utterance, the fields joined by '|'."""
    with open(join(out_dir, "train.txt"), "w", encoding="utf-8") as f:
        for m in metadata:
            f.write("|".join(str(x) for x in m) + "\n")


def build_from_path(in_dir, out_dir, sample_rate=22050, fft_size=1024, hop_size=256, n_mels=80, batch_clips=64, device="cuda:0"):
    """ljspeech.py:15-27: the LJSpeech layout -- `metadata.csv` lines `id|raw text|normalised text`, audio in `wavs/<id>.wav`;
    the normalised text is kept.  Writes the .npy files and train.txt into out_dir and returns the metadata."""
    wavs, texts = [], []
    with open(join(in_dir, "metadata.csv"), encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            parts = line.strip().split("|")
            wavs.append(join(in_dir, "wavs", "%s.wav" % parts[0]))
            texts.append(parts[2])
    metadata = process_utterances(wavs, texts, out_dir, "ljspeech", 1, None, sample_rate, fft_size, hop_size, n_mels, batch_clips, device)
    write_metadata(metadata, out_dir)
    return metadata


def build_from_path_cmu_arctic(in_dir, out_dir, speakers=CMU_ARCTIC_SPEAKERS, trim_top_db=20.0, sample_rate=22050, fft_size=1024,
                               hop_size=256, n_mels=80, batch_clips=64, device="cuda:0"):
    """cmu_arctic.py:18-32: the CMU Arctic layout -- `cmu_us_<speaker>_arctic/wav/*.wav` under in_dir (16 kHz recordings,
    resampled to sample_rate), the speakers in the order given, each one's files sorted; the speaker id is the index in
    `speakers`, the text "N/A", the numbering runs from 1 over all speakers.  Each clip is trimmed with trim_top_db (None: not
    at all).  Writes the .npy files and train.txt (fifth field: the speaker id) into out_dir and returns the metadata."""
    wavs, ids = [], []
    for sid, speaker in enumerate(speakers):
        d = join(in_dir, "cmu_us_%s_arctic" % speaker, "wav")
        if not os.path.isdir(d):
            raise FileNotFoundError(f"build_from_path_cmu_arctic: speaker {speaker!r} has no directory {d}")
        files = sorted(f for f in os.listdir(d) if f.endswith(".wav"))
        wavs += [join(d, f) for f in files]
        ids += [sid] * len(files)
    metadata = process_utterances(wavs, ["N/A"] * len(wavs), out_dir, "cmu_arctic", 1, ids, sample_rate, fft_size, hop_size, n_mels,
                                  batch_clips, device, resample=True, trim_top_db=trim_top_db)
    write_metadata(metadata, out_dir)
    return metadata
