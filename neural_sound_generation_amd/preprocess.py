"""Waveforms -> the on-disk training format that data.py reads: the reference's preprocessing (src/preprocess.py:32-35
write_metadata, src/ljspeech.py:15-102 build_from_path / _process_utterance with input_type="raw") restated without its
absent dependencies (librosa, lws, nnmnkwii, TF-1 hparams).

Per utterance, as the reference: rescale to a peak of 0.999 (hparams_tacotron.py rescaling, rescaling_max); the mel
spectrogram (N, n_mels) float32 (audio.melspectrogram: one HIP kernel, the utterances sorted by length and sent in ragged
batches); the audio zero-padded by lws_pad_lr and cut to N * hop_size samples -- the reference pads the audio the way lws
would while it frames the mel with librosa; that mismatch is kept, it defines `timesteps`; `<name>-audio-%05d.npy`,
`<name>-mel-%05d.npy`, and one `train.txt` line `audio|mel|timesteps|text[|speaker]`.

Not restated: resampling (a file at another rate is an error), silence trimming, the mu-law input types, a process pool
and the CLI.  parity unpinned, as for the rest of audio.py: tests hold the files to an fp64 restatement of the formulas.
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


def process_utterances(wavs, texts, out_dir, name="ljspeech", start_index=1, speaker_ids=None, sample_rate=22050, fft_size=1024,
                       hop_size=256, n_mels=80, batch_clips=64, device="cuda:0"):
    """ljspeech._process_utterance over a list.  wavs: paths of PCM files (audio.load_wav) or 1-D float arrays; texts: one
    string each; speaker_ids: optional integers, appended as a fifth field.  Utterance i is written as
    `<name>-audio-%05d.npy` / `<name>-mel-%05d.npy` with number start_index + i.  Returns the metadata tuples
    (audio_filename, mel_filename, timesteps, text[, speaker]) in the order given.  The files do not depend on batch_clips."""
    if len(texts) != len(wavs) or (speaker_ids is not None and len(speaker_ids) != len(wavs)):
        raise ValueError("process_utterances: wavs, texts and speaker_ids must have one entry per utterance")
    if batch_clips < 1:
        raise ValueError("process_utterances: batch_clips must be at least 1")
    os.makedirs(out_dir, exist_ok=True)
    clips = []
    for i, w in enumerate(wavs):
        label = str(w) if isinstance(w, (str, os.PathLike)) else f"utterance {i}"
        wav = audio.load_wav(w, sample_rate) if isinstance(w, (str, os.PathLike)) else np.asarray(w, dtype=np.float32)
        if wav.ndim != 1 or len(wav) <= fft_size // 2:
            raise ValueError(f"{label}: {wav.shape} samples; need a 1-D clip longer than fft_size / 2 = {fft_size // 2}")
        peak = float(np.abs(wav).max())
        if not peak > 0.0 or not np.isfinite(peak):
            raise ValueError(f"{label}: an all-zero (or non-finite) clip cannot be rescaled")
        clips.append((wav / peak * RESCALING_MAX).astype(np.float32))
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
            row = (audio_filename, mel_filename, len(out), texts[i])
            metadata[i] = row + (int(speaker_ids[i]),) if speaker_ids is not None else row
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
