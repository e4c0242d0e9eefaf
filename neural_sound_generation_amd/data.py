"""On-disk input format and batching of the reference, restated without its absent
dependencies (nnmnkwii, librosa, TF-1 hparams): CPU-side Python/numpy only, feeding the HIP path through pinned
host buffers.

Format (written by the reference's preprocessing, src/preprocess.py:32-35, src/ljspeech.py:91-102,
src/cmu_arctic.py:120-128): `<data_root>/train.txt`, one utterance per line, 4 or 5 fields separated by "|":

    <audio .npy> | <mel .npy> | <timesteps> | <text> [ | <speaker id> ]

audio: (timesteps,) array, mel: (frames, 80) float32 array, timesteps = frames * hop_size.

Pieces (names and behaviour follow src/dataloader.py:97-202,324-434):
  * `MelSpecDataSource` / `RawAudioDataSource` -- parse train.txt, lengths, speaker ids, the train / test split
    (sklearn's train_test_split with the reference's random_state=1234, test_size=0.05);
  * `PartialyRandomizedSimilarTimeLengthSampler` -- sort by length, shuffle inside groups of 32 batches, permute batches;
  * `collate_fn` -- random crop to `max_time_steps` aligned to the hop size, zero-pad to the longest item:
    returns the reference's 5-tuple (x, y, c, g, input_lengths) with c (B, 80, T) channel-first;
  * `get_data_loaders` -- {"train", "test"} loaders;  `DevicePrefetcher` -- pinned-memory, side-stream H2D copies so
    the next batch's mel is resident when the step starts (the timed path of bench.py assumes resident inputs);
  * `ResidentMelCorpus` / `plan_batch` / `ResidentMelLoader` / `get_resident_loaders` -- the same loaders with the whole mel
    corpus in device memory: an epoch's crops are planned here (the sampler and `Collate`'s rule, so equal seeds give the host
    loader's batches bit for bit), uploaded once, and a batch is one launch of csrc/collate.hip (ops.collate_mels).
    `ResidentMelCorpus.track_f0` keeps every clip's F0 track beside the mels; `ResidentMelLoader(f0=)` /
    `get_resident_loaders(f0=)` then add the F0-conditioned decoder's bins to each batch (ops.collate_f0_bins, one launch).
    `ResidentMelCorpus.keep_audio` keeps the clips' samples as well; `ResidentMelLoader(audio=True)` / `get_resident_loaders(
    audio=True)` then yield the host loader's x and y too (ops.collate_audio, one launch), which pitch-perturbed training needs.

parity unpinned: the reference's loader cannot be imported here (ordinary missing dependencies); tests/test_host_logic.py
checks the format invariants on a synthetic data root.
"""
from __future__ import annotations

import os
import random
from os.path import join
from typing import List, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.sampler import Sampler

HOP_SIZE = 256          # src/main.py:167-170, src/hparams.py: frames -> samples
NUM_MELS = 80


class _NPYDataSource:
    """One column of train.txt as a list of .npy paths (src/dataloader.py:97-152)."""

    def __init__(self, data_root: str, col: int, speaker_id: Optional[int] = None, train: bool = True,
                 test_size: Optional[float] = 0.05, test_num_samples: Optional[int] = None, random_state: int = 1234):
        self.data_root, self.col = data_root, col
        self.speaker_id = speaker_id
        self.train, self.test_size, self.test_num_samples, self.random_state = train, test_size, test_num_samples, random_state
        self.lengths: List[int] = []
        self.multi_speaker = False
        self.speaker_ids: Optional[List[int]] = None
        self.paths = self.collect_files()

    def interest_indices(self, n: int) -> np.ndarray:
        from sklearn.model_selection import train_test_split
        indices = np.arange(n)
        test_size = self.test_num_samples / n if self.test_size is None else self.test_size
        train_idx, test_idx = train_test_split(indices, test_size=test_size, random_state=self.random_state)
        return train_idx if self.train else test_idx

    def collect_files(self) -> List[str]:
        with open(join(self.data_root, "train.txt"), "rb") as f:
            rows = [ln.decode("utf-8").rstrip("\n").split("|") for ln in f.readlines() if ln.strip()]
        if not rows:
            raise ValueError(f"{self.data_root}/train.txt is empty")
        if len(rows[0]) not in (4, 5):
            raise ValueError("train.txt: expected 4 or 5 fields separated by '|', got %d" % len(rows[0]))
        self.multi_speaker = len(rows[0]) == 5
        lengths = np.array([int(r[2]) for r in rows])
        paths = np.array([join(self.data_root, r[self.col]) for r in rows])
        speakers = np.array([int(r[-1]) for r in rows]) if self.multi_speaker else None
        if self.multi_speaker and self.speaker_id is not None:      # one speaker of a multi-speaker set
            keep = speakers == self.speaker_id
            paths, lengths, speakers = paths[keep], lengths[keep], None
            self.multi_speaker = False
        idx = self.interest_indices(len(paths))
        self.lengths = [int(v) for v in lengths[idx]]
        if speakers is not None:
            self.speaker_ids = [int(v) for v in speakers[idx]]
        return [str(p) for p in paths[idx]]

    def collect_features(self, path: str) -> np.ndarray:
        return np.load(path, allow_pickle=False)

    def __len__(self):
        return len(self.paths)


class RawAudioDataSource(_NPYDataSource):
    def __init__(self, data_root, **kwargs):
        super().__init__(data_root, 0, **kwargs)


class MelSpecDataSource(_NPYDataSource):
    def __init__(self, data_root, **kwargs):
        super().__init__(data_root, 1, **kwargs)


class PartialyRandomizedSimilarTimeLengthSampler(Sampler):
    """Sort by length, shuffle inside groups of `batch_group_size`, permute whole batches (src/dataloader.py:158-202):
    a batch holds clips of similar length, so little of it is padding."""

    def __init__(self, lengths, batch_size=16, batch_group_size=None, permutate=True):
        self.lengths, self.sorted_indices = torch.sort(torch.LongTensor(lengths))
        self.batch_size = batch_size
        if batch_group_size is None:
            batch_group_size = min(batch_size * 32, len(self.lengths))
            if batch_group_size % batch_size != 0:
                batch_group_size -= batch_group_size % batch_size
        self.batch_group_size = max(batch_group_size, 0)
        self.permutate = permutate

    def __iter__(self):
        indices = self.sorted_indices.clone().tolist()
        g = self.batch_group_size
        e = 0
        if g > 0:
            for i in range(len(indices) // g):
                s, e = i * g, (i + 1) * g
                chunk = indices[s:e]
                random.shuffle(chunk)
                indices[s:e] = chunk
            if self.permutate and e > 0:
                batches = [indices[i:i + self.batch_size] for i in range(0, e, self.batch_size)]
                random.shuffle(batches)
                indices[:e] = [i for b in batches for i in b]
        tail = indices[e:]
        random.shuffle(tail)
        indices[e:] = tail
        return iter(indices)

    def __len__(self):
        return len(self.sorted_indices)


class MelDataset(Dataset):
    """(raw audio or None, mel (frames, 80), speaker id or None) per utterance (src/dataloader.py:205-229)."""

    def __init__(self, mel: MelSpecDataSource, audio: Optional[RawAudioDataSource] = None):
        self.mel, self.audio = mel, audio
        self.multi_speaker = mel.multi_speaker
        self.lengths = mel.lengths

    def __getitem__(self, idx):
        c = self.mel.collect_features(self.mel.paths[idx])
        if c.ndim != 2 or c.shape[1] != NUM_MELS:
            raise ValueError(f"{self.mel.paths[idx]}: expected a (frames, {NUM_MELS}) array, got {c.shape}")
        x = self.audio.collect_features(self.audio.paths[idx]) if self.audio is not None else None
        g = self.mel.speaker_ids[idx] if self.multi_speaker else None
        return x, c.astype(np.float32, copy=False), g

    def __len__(self):
        return len(self.mel)


def ensure_divisible(length, divisible_by=HOP_SIZE, lower=True):
    if length % divisible_by == 0:
        return length
    return length - length % divisible_by if lower else length + (divisible_by - length % divisible_by)


class Collate:
    """collate_fn of src/dataloader.py:324-434 for the local-conditioning (mel) case with upsampled features: crop
    every utterance to at most `max_time_steps` samples = max_time_steps // hop frames at a random frame-aligned
    offset, zero-pad to the longest in the batch.  Returns (x, y, c, g, input_lengths):
      x (B, 1, Tx) float32 audio or None, y (B, Tx, 1) or None, c (B, 80, Tc) float32, g (B,) int64 or None,
      input_lengths (B,) int64 = audio samples per item (frames * hop when there is no audio)."""

    def __init__(self, max_time_steps: Optional[int] = None, hop_size: int = HOP_SIZE, frame_multiple: int = 1,
                 rng: Optional[np.random.RandomState] = None):
        self.max_time_steps, self.hop = max_time_steps, hop_size
        self.frame_multiple = frame_multiple          # e.g. 4: every clip's frame count is cut to a multiple of the model's stride
        self.rng = rng if rng is not None else np.random

    def __call__(self, batch):
        items = []
        for x, c, g in batch:
            frames = len(c)
            if x is not None and len(x) != frames * self.hop:
                raise ValueError("audio and mel lengths disagree: %d samples vs %d frames x hop %d" % (len(x), frames, self.hop))
            if self.max_time_steps is not None:
                max_frames = ensure_divisible(self.max_time_steps, self.hop, True) // self.hop
                if frames > max_frames:
                    s = self.rng.randint(0, frames - max_frames)      # (the reference's exclusive upper bound)
                    c = c[s:s + max_frames]
                    if x is not None:
                        x = x[s * self.hop:(s + max_frames) * self.hop]
            if self.frame_multiple > 1 and len(c) >= self.frame_multiple:
                keep = len(c) - len(c) % self.frame_multiple
                c = c[:keep]
                if x is not None:
                    x = x[:keep * self.hop]
            items.append((x, c, g))
        has_audio = items[0][0] is not None
        input_lengths = [len(x) if has_audio else len(c) * self.hop for x, c, _ in items]
        max_frames = max(len(c) for _, c, _ in items)
        c_batch = np.zeros((len(items), max_frames, NUM_MELS), dtype=np.float32)
        for i, (_, c, _) in enumerate(items):
            c_batch[i, :len(c)] = c
        c_t = torch.from_numpy(c_batch).transpose(1, 2).contiguous()             # (B, 80, T)
        x_t = y_t = None
        if has_audio:
            max_len = max(input_lengths)
            x_batch = np.zeros((len(items), max_len), dtype=np.float32)
            for i, (x, _, _) in enumerate(items):
                x_batch[i, :len(x)] = x
            x_t = torch.from_numpy(x_batch).unsqueeze(1).contiguous()             # (B, 1, T)
            y_t = torch.from_numpy(x_batch).unsqueeze(-1).contiguous()            # (B, T, 1)
        g_t = torch.LongTensor([g for _, _, g in items]) if items[0][2] is not None else None
        return x_t, y_t, c_t, g_t, torch.LongTensor(input_lengths)


def get_data_loaders(data_root: str, batch_size: int, max_time_steps: Optional[int] = None, speaker_id=None, num_workers: int = 2,
                     with_audio: bool = False, test_size=0.05, test_num_samples=None, random_state: int = 1234,
                     pin_memory: bool = True, frame_multiple: int = 1):
    """{"train": loader, "test": loader} over `data_root` (src/dataloader.py get_data_loaders).  The train loader uses
    the length-bucketed sampler; both crop / pad through `Collate`."""
    loaders = {}
    for phase in ("train", "test"):
        train = phase == "train"
        kw = dict(speaker_id=speaker_id, train=train, test_size=test_size, test_num_samples=test_num_samples, random_state=random_state)
        mel = MelSpecDataSource(data_root, **kw)
        audio = RawAudioDataSource(data_root, **kw) if with_audio else None
        ds = MelDataset(mel, audio)
        sampler = PartialyRandomizedSimilarTimeLengthSampler(ds.lengths, batch_size=batch_size) if train else None
        loaders[phase] = DataLoader(ds, batch_size=batch_size, sampler=sampler, shuffle=False, num_workers=num_workers,
                                    collate_fn=Collate(max_time_steps, frame_multiple=frame_multiple), pin_memory=pin_memory)
    return loaders


class DevicePrefetcher:
    """Wraps a loader of (x, y, c, g, input_lengths): copies the NEXT batch's c (and g) to the GPU on a side stream from
    pinned memory while the current step runs, and hands out batches whose tensors are already resident."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)

    def _stage(self, batch):
        x, y, c, g, lens = batch
        with torch.cuda.stream(self.stream):
            c = (c if c.is_pinned() else c.pin_memory()).to(self.device, non_blocking=True)
            if g is not None:
                g = g.to(self.device, non_blocking=True)
        return x, y, c, g, lens

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while True:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            cur = nxt
            cur[2].record_stream(torch.cuda.current_stream(self.device))
            try:
                nxt = self._stage(next(it))
            except StopIteration:
                yield cur
                return
            yield cur

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset


# ------------------------------------------------------------------------------------------------
# The corpus resident in device memory: batches built by one kernel, no host work or copy per step
# ------------------------------------------------------------------------------------------------

class ResidentMelCorpus:
    """Every mel of a `MelSpecDataSource`, read once and kept in ONE tensor on `device`: `frames` (sum of frames, 80) fp32,
    frame-major -- the clips' on-disk arrays concatenated (LJSpeech: ~2.4 GB).  On the host: `offsets` (n + 1,) int64, clip i is
    frames[offsets[i]:offsets[i + 1]]; `n_frames` (n,) int64; `lengths`, the source's `timesteps` column (what the sampler sorts
    by).  `speaker_ids` (n,) int64 on `device` for a multi-speaker root, else None.  The arrays are read into host memory
    first (the corpus' size of it, freed afterwards) and staged through a pinned chunk.  device "cpu" keeps `frames` on the
    host: enough for planning and for tests, not for `ResidentMelLoader`'s batches (ops.collate_mels has no CPU path).
    `f0`, `f0_sums`, `f0_settings`: None until `track_f0` has put the clips' F0 tracks beside the mels.
    `audio`, `audio_hop`: None until `keep_audio` has put the clips' samples there too."""

    CHUNK_FRAMES = 1 << 16          # the pinned staging buffer: 65 536 frames = 21 MB

    def __init__(self, mel_source: MelSpecDataSource, device="cuda:0"):
        self.device = torch.device(device)
        self.multi_speaker = mel_source.multi_speaker
        self.lengths = list(mel_source.lengths)
        arrays = []
        for path in mel_source.paths:
            c = mel_source.collect_features(path)
            if c.ndim != 2 or c.shape[1] != NUM_MELS:
                raise ValueError(f"{path}: expected a (frames, {NUM_MELS}) array, got {c.shape}")
            arrays.append(c.astype(np.float32, copy=False))
        self.n_frames = np.array([len(c) for c in arrays], dtype=np.int64)
        self.offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(self.n_frames, dtype=np.int64)])
        total = int(self.offsets[-1])
        self.frames = torch.empty(total, NUM_MELS, dtype=torch.float32, device=self.device)
        self._upload(arrays, self.frames, self.CHUNK_FRAMES)
        self.speaker_ids = (torch.tensor(mel_source.speaker_ids, dtype=torch.int64, device=self.device)
                            if self.multi_speaker else None)
        self.f0 = self.f0_sums = self.f0_settings = None
        self.audio = self.audio_hop = None

    def keep_audio(self, audio_source: RawAudioDataSource, hop_size: int = HOP_SIZE):
        """Keep every clip's waveform beside the mels: `audio` (total_frames * hop_size,) fp32 on the corpus' device, the clips'
        on-disk audio arrays concatenated in the mels' order, so that clip i is audio[offsets[i] * hop_size : offsets[i + 1] *
        hop_size] and a batch's x is a crop by the plan rows collate_mels takes (ops.collate_audio, `ResidentMelLoader(audio=True)`);
        `audio_hop` = hop_size.  `audio_source`: a `RawAudioDataSource` over the same split as the mels (clip i is its path i;
        ValueError, `Collate`'s, where len(x) != frames * hop_size).  Each clip is read once and staged through a pinned chunk, one
        clip in host memory at a time; device "cpu" keeps the array on the host (planning, host tests).  The samples stay fp32 --
        the host loader's x is the file's fp32 and the batches are to equal it bit for bit --, 1 024 bytes a frame beside the mels'
        320: LJSpeech is about 7.6 GB of samples beside 2.4 GB of mels."""
        if isinstance(hop_size, bool) or not isinstance(hop_size, (int, np.integer)) or hop_size < 1:
            raise ValueError(f"ResidentMelCorpus.keep_audio: hop_size must be a positive integer, got {hop_size!r}")
        if len(audio_source.paths) != len(self):
            raise ValueError(f"ResidentMelCorpus.keep_audio: {len(audio_source.paths)} audio clips for {len(self)} mels: not the same split")
        hop_size = int(hop_size)

        def clips():
            for i, path in enumerate(audio_source.paths):
                x = audio_source.collect_features(path)
                if x.ndim != 1 or len(x) != int(self.n_frames[i]) * hop_size:
                    raise ValueError("audio and mel lengths disagree: %d samples vs %d frames x hop %d" % (len(x), int(self.n_frames[i]), hop_size))
                yield x
        samples = torch.empty(int(self.offsets[-1]) * hop_size, dtype=torch.float32, device=self.device)
        self._upload(clips(), samples, self.CHUNK_FRAMES * NUM_MELS)           # (the mels' staging size)
        self.audio, self.audio_hop = samples, hop_size
        return self

    def track_f0(self, audio_source: Optional[RawAudioDataSource] = None, tracker="yin", tracker_options=None, fmin=65.0, fmax=500.0, group_clips=64,
                 group_samples=1 << 24, hop_size: int = HOP_SIZE):
        """Track every clip's F0 ONCE and keep it beside the mels: F0 frame t is mel frame t, and a frame's value depends on its
        own samples alone, so a batch's track is a crop of the clip's by the plan rows collate_mels takes (ops.collate_f0_bins) and
        no tracker runs in the training loop.  `audio_source`: a `RawAudioDataSource` over the same split as the mels (clip i is
        its path i; ValueError, `Collate`'s, where len(x) != frames * hop_size).  The clips are tracked whole, in zero-padded
        groups of at most `group_clips` clips and at most `group_samples` padded samples (a longer clip is a group of its own), by
        audio.f0 (tracker="yin") or audio.f0_track ("viterbi", tracker_options: its costs) over [fmin, fmax] Hz, as
        evaluate._f0_tracker names and checks them; of a clip's 1 + len // hop_size frames the first n_frames[i] are kept.  Sets
          f0          (total_frames,) fp32 on the device, Hz, +0.0 where unvoiced: clip i is f0[offsets[i]:offsets[i + 1]];
          f0_sums     (n, 3) fp64 numpy: audio.logf0_sums of each clip's kept frames (of the row f0[offsets[i]:offsets[i + 1]]);
          f0_settings {"tracker", "tracker_options", "fmin", "fmax"}.
        Both trackers give a clip's track independent of the batch it is tracked in, so none of this depends on the grouping.  The
        audio is not kept.  AGAINST THE HOST PATH (train.train_conditioned tracking a batch's cropped audio): the crop there is
        zero outside itself, here the frames at a crop's edges see the clip's real neighbours.  With "yin", crop frame t of count
        frames is bit for bit the host path's where t * hop - 512 >= 0 and t * hop + 511 + tau_max <= count * hop - 1 (tau_max:
        audio.f0_lags; at the defaults frames 2 .. count - 4); "viterbi" is a path over the whole clip and promises no such
        equality.
        audio_source=None over a corpus with resident audio (`keep_audio`; ValueError without it, or where hop_size is not its
        audio_hop): nothing is read from disk -- a group's zero-padded rows are one ops.collate_audio launch on whole-clip plan
        rows (i, offsets[i], n_frames[i]), the groups follow the same rule, and f0, f0_sums and f0_settings are bit for bit those
        of track_f0(audio_source)."""
        from . import audio, ops
        from .evaluate import _f0_tracker
        track = _f0_tracker("ResidentMelCorpus.track_f0", tracker, tracker_options)
        audio.f0_lags(22050, fmin, fmax)                                     # (the range, checked before anything is read)
        if audio_source is None:
            if self.audio is None:
                raise ValueError("ResidentMelCorpus.track_f0: no audio_source and the corpus keeps no audio (keep_audio)")
            if hop_size != self.audio_hop:
                raise ValueError(f"ResidentMelCorpus.track_f0: hop_size = {hop_size}, the resident audio's is {self.audio_hop}")
        elif len(audio_source.paths) != len(self):
            raise ValueError(f"ResidentMelCorpus.track_f0: {len(audio_source.paths)} audio clips for {len(self)} mels: not the same split")
        if group_clips < 1 or group_samples < 1:
            raise ValueError("ResidentMelCorpus.track_f0: group_clips and group_samples must be positive")
        f0_all = torch.empty(int(self.offsets[-1]), dtype=torch.float32, device=self.device)
        group, first = [], 0                                                 # the waiting clips' audio; the index of the first of them

        def flush():
            nonlocal group, first
            lens = np.array([len(x) for x in group], dtype=np.int64)
            if audio_source is None:                                         # (a group of empty clips: one frame of zeros, none kept)
                clips = np.arange(first, first + len(group), dtype=np.int64)
                rows = np.stack((clips, self.offsets[clips], self.n_frames[clips]), axis=1)
                wav = ops.collate_audio(self.audio, torch.from_numpy(rows), max(1, int(self.n_frames[clips].max())), hop_size)
            else:
                wav = np.zeros((len(group), max(1, int(lens.max()))), dtype=np.float32)
                for j, x in enumerate(group):
                    wav[j, :len(x)] = x
                wav = torch.from_numpy(wav).to(self.device)
            f0, _ = track(wav, hop_size=hop_size, fmin=fmin, fmax=fmax, lengths=lens)
            keep = torch.from_numpy(self.n_frames[first:first + len(group)]).to(self.device)
            mask = torch.arange(f0.shape[1], device=self.device).unsqueeze(0) < keep.unsqueeze(1)
            f0_all[int(self.offsets[first]):int(self.offsets[first + len(group)])] = f0[mask]      # row-major: the clips in order
            group, first = [], first + len(group)

        for i in range(len(self)):
            if audio_source is None:
                x = range(int(self.n_frames[i]) * hop_size)                  # (its length is all the grouping rule and flush need)
            else:
                x = audio_source.collect_features(audio_source.paths[i])
                if x.ndim != 1 or len(x) != int(self.n_frames[i]) * hop_size:
                    raise ValueError("audio and mel lengths disagree: %d samples vs %d frames x hop %d" % (len(x), int(self.n_frames[i]), hop_size))
            widest = max([len(x)] + [len(v) for v in group])
            if group and (len(group) + 1 > group_clips or (len(group) + 1) * widest > group_samples):
                flush()
            group.append(x if audio_source is None else x.astype(np.float32, copy=False))
        if group:
            flush()
        # (per clip, on its own row: torch's sum over a row may depend on the row's width, and nothing here may depend on the groups)
        sums = [audio.logf0_sums(f0_all[int(a):int(b)].unsqueeze(0)) if b > a else torch.zeros(1, 3, dtype=torch.float64, device=self.device)
                for a, b in zip(self.offsets[:-1], self.offsets[1:])]
        self.f0_sums = (torch.cat(sums).cpu().numpy() if sums else np.zeros((0, 3)))
        self.f0 = f0_all
        self.f0_settings = {"tracker": tracker, "tracker_options": dict(tracker_options or {}), "fmin": float(fmin), "fmax": float(fmax)}
        return self

    def speaker_f0_stats(self, n_speakers: int):
        """evaluate.speaker_f0_stats from the resident track: `f0_sums` pooled per speaker in fp64 on the host -> (stats
        (n_speakers, 2) fp64: mean and (population) standard deviation of log2 F0 over the speaker's voiced kept frames, NaN for
        a speaker without one; counts (n_speakers,) int64), torch tensors on the host.  A root without speaker ids is speaker 0."""
        if self.f0_sums is None:
            raise ValueError("ResidentMelCorpus.speaker_f0_stats: the corpus has no F0 track (track_f0)")
        if isinstance(n_speakers, bool) or not isinstance(n_speakers, (int, np.integer)) or n_speakers < 1:
            raise ValueError(f"speaker_f0_stats: n_speakers must be a positive integer, got {n_speakers!r}")
        g = self.speaker_ids.cpu().numpy() if self.speaker_ids is not None else np.zeros(len(self), dtype=np.int64)
        if len(g) and (g.min() < 0 or g.max() >= n_speakers):
            raise ValueError(f"speaker_f0_stats: the corpus' speaker ids are not all in [0, {n_speakers})")
        total = np.zeros((n_speakers, 3), dtype=np.float64)
        np.add.at(total, g, self.f0_sums)
        n, s1, s2 = (torch.from_numpy(total[:, k].copy()) for k in range(3))
        mean = s1 / n                                                           # (0 / 0: NaN for a speaker without a voiced frame)
        std = torch.sqrt(torch.clamp(s2 / n - mean * mean, min=0.0))
        return torch.stack((mean, std), dim=1), n.to(torch.int64)

    def _upload(self, arrays, dst, chunk_rows):
        """The rows of `arrays` (an iterable, read one at a time), in order, into `dst` through a pinned chunk of `chunk_rows` rows."""
        cuda = self.device.type == "cuda"
        stage = torch.empty(chunk_rows, *dst.shape[1:], dtype=torch.float32, pin_memory=cuda)
        stage_np = stage.numpy()
        done = fill = 0                                      # rows already on the device / waiting in the chunk

        def flush():
            nonlocal done, fill
            dst[done:done + fill].copy_(stage[:fill])            # blocking: the chunk is free again when it returns
            done, fill = done + fill, 0

        for c in arrays:
            at = 0
            while at < len(c):
                n = min(len(c) - at, chunk_rows - fill)
                stage_np[fill:fill + n] = c[at:at + n]
                at, fill = at + n, fill + n
                if fill == chunk_rows:
                    flush()
        if fill:
            flush()

    def __len__(self):
        return len(self.n_frames)


def plan_batch(n_frames_of_items, max_time_steps: Optional[int], hop_size: int, frame_multiple: int, rng):
    """`Collate.__call__`'s crop rule for items of these frame counts, in its order and with its draws from `rng`: per item
    (s, count) -- the item is frames [s, s + count) of its clip.  Host only."""
    s_out, count_out = [], []
    for frames in n_frames_of_items:
        s, count = 0, int(frames)
        if max_time_steps is not None:
            max_frames = ensure_divisible(max_time_steps, hop_size, True) // hop_size
            if count > max_frames:
                s = int(rng.randint(0, count - max_frames))      # drawn only for a clip that is cropped, in item order
                count = max_frames
        if frame_multiple > 1 and count >= frame_multiple:
            count -= count % frame_multiple
        s_out.append(s)
        count_out.append(count)
    return np.array(s_out, dtype=np.int64), np.array(count_out, dtype=np.int64)


class EpochPlan:
    """One epoch of a `ResidentMelLoader` as the host knows it: `plan` (n_batches, B_max, 3) int64 rows of (clip, first corpus
    frame, frames) -- rows past a short batch's size are zeros and are never launched --, `sizes` (n_batches,) items per batch,
    `widths` (n_batches,) = the batch's longest item = its T."""

    def __init__(self, plan, sizes, widths):
        self.plan, self.sizes, self.widths = plan, sizes, widths

    def __len__(self):
        return len(self.sizes)


class ResidentMelLoader:
    """The loader of `get_data_loaders` + `DevicePrefetcher` over a `ResidentMelCorpus`: yields (None, None, c, g,
    input_lengths) with c (B, 80, T) fp32 on the device (a fresh tensor per batch), g (B,) int64 on the device or None,
    input_lengths (B,) int64 on the CPU = frames * hop.  With equal seeds (Python's `random` for the order, `rng` for the crops)
    the batches are the host loader's, bit for bit: the epoch's order comes from the same sampler class (train) or is sequential
    with a smaller last batch (test), the crops from `plan_batch`.

    `__iter__` plans the whole epoch on the host, checks the plan and uploads it once; a step is then one ops.collate_mels
    launch on the current stream with T = the batch's longest item, and one gather of speaker ids: nothing is copied from the
    host and nothing is synchronised per step.

    shard=(rank, world): this rank takes the batches k with k % world == rank among the first (n_batches // world) * world
    batches of the epoch; the remaining n_batches % world batches are DROPPED, so that every rank runs the same number of steps
    (the gradient all-reduce would hang otherwise).  Every rank must seed Python's `random` and `rng` alike: all of them draw
    the same order and the same plan, then keep their share.  len() is then the rank's number of batches.

    f0=(n_bins, fmin, fmax), over a corpus with an F0 track (`ResidentMelCorpus.track_f0`; ValueError here without one): a batch
    is the six-tuple (None, None, c, g, input_lengths, f0_bins) with f0_bins (B, T // 4) int64 on the device, the F0-conditioned
    decoder's bins of the batch's crops (one ops.collate_f0_bins launch on the plan rows already on the device; T < 4: an empty
    (B, 0) tensor and no launch), which train.train_conditioned, evaluate.test_conditioned and epoch.run_conditioned_epoch take as
    they come.  The first five elements and the draws from `random` and `rng` are those of the loader without f0.  The bins are
    crops of the WHOLE clip's track: see track_f0 for where they are, and are not, the host path's.

    audio=True, over a corpus with resident audio (`ResidentMelCorpus.keep_audio`; ValueError here without it, or where hop_size
    is not its audio_hop): the first two elements are x (B, 1, T * hop) and y (B, T * hop, 1) fp32 on the device, two views of one
    fresh tensor -- one ops.collate_audio launch on the plan rows already on the device.  With equal seeds they are
    get_data_loaders(with_audio=True)'s x and y bit for bit; c, g, input_lengths, the optional f0_bins and the draws from
    `random` and `rng` are exactly those of the loader without audio.  train.train_conditioned(pitch_perturb=) runs on such
    batches."""

    def __init__(self, corpus: ResidentMelCorpus, batch_size: int, max_time_steps: Optional[int] = None, frame_multiple: int = 1,
                 train: bool = True, rng=None, shard=None, hop_size: int = HOP_SIZE, f0=None, audio: bool = False):
        if batch_size < 1:
            raise ValueError("ResidentMelLoader: batch_size < 1")
        if audio:
            if getattr(corpus, "audio", None) is None:
                raise ValueError("ResidentMelLoader: audio=True over a corpus without resident audio (ResidentMelCorpus.keep_audio)")
            if hop_size != corpus.audio_hop:
                raise ValueError(f"ResidentMelLoader: hop_size = {hop_size}, the corpus' resident audio has hop {corpus.audio_hop}")
        self.audio = bool(audio)
        if f0 is not None:
            if len(f0) != 3 or isinstance(f0[0], bool) or not isinstance(f0[0], (int, np.integer)) or f0[0] < 1 or not 0 < f0[1] < f0[2] < float("inf"):
                raise ValueError(f"ResidentMelLoader: f0 = {f0!r} is not (n_bins, fmin, fmax) with n_bins >= 1 and 0 < fmin < fmax")
            if getattr(corpus, "f0", None) is None:
                raise ValueError("ResidentMelLoader: f0 given over a corpus without an F0 track (ResidentMelCorpus.track_f0)")
            f0 = (int(f0[0]), float(f0[1]), float(f0[2]))
        self.f0 = f0
        if shard is not None and not (len(shard) == 2 and shard[1] >= 1 and 0 <= shard[0] < shard[1]):
            raise ValueError(f"ResidentMelLoader: shard = {shard} is not (rank, world) with 0 <= rank < world")
        self.dataset = corpus
        self.batch_size, self.max_time_steps, self.frame_multiple, self.hop = batch_size, max_time_steps, frame_multiple, hop_size
        self.train, self.shard = train, shard
        self.rng = rng if rng is not None else np.random
        self.sampler = PartialyRandomizedSimilarTimeLengthSampler(corpus.lengths, batch_size=batch_size) if train else None

    def __len__(self):
        n = -(-len(self.dataset) // self.batch_size)
        return n if self.shard is None else n // self.shard[1]

    def plan_epoch(self) -> EpochPlan:
        """Draw the epoch's order and crops (host only; consumes `random` and `rng` exactly as iterating the host loader does)."""
        corpus, bs = self.dataset, self.batch_size
        order = list(iter(self.sampler)) if self.train else list(range(len(corpus)))
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        plan = np.zeros((len(batches), bs, 3), dtype=np.int64)
        sizes = np.array([len(b) for b in batches], dtype=np.int64)
        widths = np.zeros(len(batches), dtype=np.int64)
        for k, clips in enumerate(batches):
            clips = np.array(clips, dtype=np.int64)
            s, count = plan_batch(corpus.n_frames[clips], self.max_time_steps, self.hop, self.frame_multiple, self.rng)
            plan[k, :len(clips), 0], plan[k, :len(clips), 1], plan[k, :len(clips), 2] = clips, corpus.offsets[clips] + s, count
            widths[k] = count.max()
        if self.shard is not None:
            rank, world = self.shard
            keep = np.arange(rank, len(batches) // world * world, world)
            plan, sizes, widths = plan[keep], sizes[keep], widths[keep]
        return EpochPlan(plan, sizes, widths)

    def __iter__(self):
        from . import ops
        corpus = self.dataset
        ep = self.plan_epoch()
        if len(ep) == 0:
            return
        ops.check_collate_plan(ep.plan, ep.widths[:, None], len(corpus.frames))
        plan_dev = torch.from_numpy(ep.plan).to(corpus.device)          # the epoch's one upload
        for k in range(len(ep)):
            B, rows = int(ep.sizes[k]), plan_dev[k, :int(ep.sizes[k])]
            c = ops.collate_mels(corpus.frames, rows, int(ep.widths[k]))
            g = corpus.speaker_ids[rows[:, 0]] if corpus.speaker_ids is not None else None
            lengths = torch.from_numpy(ep.plan[k, :B, 2] * self.hop)
            T = int(ep.widths[k])
            x = y = None
            if self.audio:
                wav = ops.collate_audio(corpus.audio, rows, T, self.hop)
                x, y = wav.unsqueeze(1), wav.unsqueeze(2)
            if self.f0 is None:
                yield x, y, c, g, lengths
                continue
            bins = (ops.collate_f0_bins(corpus.f0, rows, T, *self.f0) if T >= 4 else
                    torch.empty(B, 0, dtype=torch.int64, device=corpus.device))
            yield x, y, c, g, lengths, bins


def get_resident_loaders(data_root: str, batch_size: int, max_time_steps: Optional[int] = None, speaker_id=None, test_size=0.05,
                         test_num_samples=None, random_state: int = 1234, frame_multiple: int = 1, device="cuda:0", rng=None,
                         shard=None, f0=None, audio: bool = False):
    """`get_data_loaders` with the corpus resident on `device`: {"train": ResidentMelLoader, "test": ResidentMelLoader} over the
    same train / test split.  `shard` applies to the train loader only.
    f0: None, or a dict {"n_bins", "fmin", "fmax"[, "tracker", "tracker_options"]} for an F0-conditioned model (n_bins and the range
    are the model's n_f0_bins and f0_range): both corpora read their split's audio once (`RawAudioDataSource`), track it
    (`ResidentMelCorpus.track_f0` with that tracker over its own default range, the one train.train_conditioned tracks a host
    batch over) and both loaders yield six-tuples with the bins (`ResidentMelLoader(f0=)`).  The audio is not kept.
    audio=True: both corpora read their split's audio once and KEEP it (`ResidentMelCorpus.keep_audio`), both loaders yield x
    and y (`ResidentMelLoader(audio=True)`: get_data_loaders(with_audio=True)'s batches), and with f0 as well the tracks come from
    the resident samples (`track_f0()` without a source), not from a second read."""
    if f0 is not None:
        f0 = dict(f0)
        if set(f0) - {"n_bins", "fmin", "fmax", "tracker", "tracker_options"} or not {"n_bins", "fmin", "fmax"} <= set(f0):
            raise ValueError(f"get_resident_loaders: f0 = {sorted(f0)} is not n_bins, fmin, fmax (and tracker, tracker_options)")
    loaders = {}
    for phase in ("train", "test"):
        train = phase == "train"
        kw = dict(speaker_id=speaker_id, train=train, test_size=test_size, test_num_samples=test_num_samples, random_state=random_state)
        corpus = ResidentMelCorpus(MelSpecDataSource(data_root, **kw), device)
        if audio:
            corpus.keep_audio(RawAudioDataSource(data_root, **kw))
        if f0 is not None:
            corpus.track_f0(None if audio else RawAudioDataSource(data_root, **kw), tracker=f0.get("tracker", "yin"), tracker_options=f0.get("tracker_options"))
        loaders[phase] = ResidentMelLoader(corpus, batch_size, max_time_steps, frame_multiple, train=train, rng=rng,
                                           shard=shard if train else None,
                                           f0=None if f0 is None else (f0["n_bins"], f0["fmin"], f0["fmax"]), audio=audio)
    return loaders


def write_synthetic_data_root(data_root: str, n_utts: int = 12, min_frames: int = 40, max_frames: int = 200, n_speakers: int = 0,
                              with_audio: bool = True, seed: int = 0, voiced: bool = False) -> None:
    """A data root in the reference's format filled with random mels in [0, 1) (tests, smoke runs: there is no network
    for LJSpeech / CMU Arctic here).  The audio is uniform noise, which a pitch tracker calls unvoiced everywhere; voiced=True
    writes instead, for clip i of n = frames * 256 samples, a gliding harmonic tone with an unvoiced tail,
        0.3 * sum_{h = 1..6} 0.6^h sin(h phase[m]),   phase = the running sum of 2 pi f[m] / 22050,
        f[m] = 110 (1 + 0.25 (i mod 4)) (1 + 0.3 m / n),
    whose last fifth is 0.006 * standard normal noise from a RandomState of its own -- the mels, the speaker ids and train.txt are
    the same either way (the audio says nothing about the random mels: it gives the F0 paths something to track)."""
    rs = np.random.RandomState(seed)
    rs_tail = np.random.RandomState([seed, 0xF0]) if voiced else None
    os.makedirs(data_root, exist_ok=True)
    lines = []
    for i in range(n_utts):
        frames = int(rs.randint(min_frames, max_frames + 1))
        mel = rs.rand(frames, NUM_MELS).astype(np.float32)
        np.save(join(data_root, "synth-mel-%05d.npy" % i), mel, allow_pickle=False)
        if with_audio:
            wav = rs.uniform(-1, 1, frames * HOP_SIZE).astype(np.float32)       # (drawn either way: the later clips' mels depend on it)
            if voiced:
                n = frames * HOP_SIZE
                f = 110.0 * (1 + 0.25 * (i % 4)) * (1 + 0.3 * np.arange(n) / n)
                phase = np.cumsum(2 * np.pi * f / 22050.0)
                tone = 0.3 * sum(0.6 ** h * np.sin(h * phase) for h in range(1, 7))
                tone[n - n // 5:] = 0.006 * rs_tail.standard_normal(n // 5)
                wav = tone.astype(np.float32)
            np.save(join(data_root, "synth-audio-%05d.npy" % i), wav, allow_pickle=False)
        fields = ["synth-audio-%05d.npy" % i, "synth-mel-%05d.npy" % i, str(frames * HOP_SIZE), "utterance %d" % i]
        if n_speakers > 0:
            fields.append(str(int(rs.randint(0, n_speakers))))
        lines.append("|".join(fields))
    with open(join(data_root, "train.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def synthetic_mel_batch(B: int, T: int, generator: torch.Generator, device, n_mels: int = 80) -> torch.Tensor:
    """(B, 1, n_mels, T) float32 in [0, 1] with the texture of a normalised mel spectrogram (the range of
    src/audio_tacotron.py:228-234): a few harmonic ridges per clip whose pitch and energy drift over the frames, a little noise.
    For convergence checks and demos without a corpus -- white noise (bench.py's timing input) cannot be
    reconstructed, so a loss on it says nothing.  No reference counterpart."""
    t = torch.linspace(0, 1, T, device=device).view(1, 1, T)
    h = torch.linspace(0, 1, n_mels, device=device).view(1, n_mels, 1)
    x = torch.zeros(B, n_mels, T, device=device)

    def u():
        return torch.rand(B, 1, 1, generator=generator, device=device)

    for _ in range(4):
        f0, drift, rate, phase = u() * 0.5 + 0.1, (u() - 0.5) * 0.3, u() * 6 + 1, u() * 6.28
        centre = f0 + drift * torch.sin(rate * 6.28 * t + phase)
        width = u() * 0.04 + 0.02
        energy = 0.5 + 0.5 * torch.sin(u() * 20 * t + phase)
        x = x + energy * torch.exp(-((h - centre) / width) ** 2)
    x = x + 0.05 * torch.randn(B, n_mels, T, generator=generator, device=device)
    return torch.sigmoid(3.0 * (x - 0.5)).unsqueeze(1).contiguous()

