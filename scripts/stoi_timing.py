"""Timing of the intelligibility figures (audio.stoi: nsg_audio_stoi_envelopes, nsg_audio_stoi_score) on 64 pairs of 10 s at 22 050 Hz
(clean: synthetic voiced clips with a pause; processed: the same plus noise at 5 dB SNR).  Reported separately, each as the median
over windows of HIP-event times on the launch stream (every call warmed up; a window is a run of whole calls between two events):
  * resample: both signals 22 050 -> 10 000 Hz (audio.resample, twice);
  * envelopes: nsg_audio_stoi_envelopes on the resampled pair (three launches);
  * score: nsg_audio_stoi_score, STOI and ESTOI;
  * whole: audio.stoi from the 22 050 Hz pair, per variant;
  * spectral_convergence of the same 64 clips' worth of frames (862 frames, n_fft 1024, hop 256) in the same run, for scale;
  * numpy: seconds per clip of the fp64 restatement (tests/helpers/stoi_ref.py) on this host's CPU, one clip.
Without --step this is the driver: every GPU step is a process of its own under `timeout -k 10 <seconds>`, the steps chained so that
the first failure ends the run; --json PATH collects the steps' records.  There is no fallback: without a GPU the GPU steps fail.
    python scripts/stoi_timing.py [--json profiles/stoi_timing.json]"""
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("numpy", 120), ("resample", 240), ("stoi", 240), ("spectral_convergence", 240))     # (step, its time limit in seconds)
SR, B, SECONDS = 22050, 64, 10
WINDOWS, MIN_WINDOW_S = 7, 0.25


def driver():
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    scratch = tempfile.mkdtemp(prefix="stoi_timing_")
    tmp = [os.path.join(scratch, f"{s}.json") for s, _ in STEPS]
    cmd = " && ".join(f"timeout -k 10 {limit} {shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --step {s} --json {shlex.quote(t)}"
                      for (s, limit), t in zip(STEPS, tmp))
    rc = subprocess.call(cmd, shell=True)
    records = []
    for t in tmp:
        if os.path.exists(t):
            with open(t) as fh:
                records.append(json.load(fh))
            os.remove(t)
    os.rmdir(scratch)
    if rc:
        raise SystemExit(f"stoi_timing: a step failed (exit status {rc}); nothing more was started")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(records, fh, indent=1)


def clips(n, rate, count):
    import numpy as np
    xs, ys = [], []
    for b in range(count):
        rs = np.random.RandomState(b)
        t = np.arange(n, dtype=np.float64)
        phase = 2 * np.pi * np.cumsum(rs.uniform(90.0, 250.0) * (1.0 + 0.2 * np.sin(2 * np.pi * t / rate)) / rate)
        x = sum(0.6 ** h * np.sin(h * phase) for h in range(1, 7)) + 0.02 * rs.standard_normal(n)
        x[int(0.7 * n):int(0.8 * n)] = 1e-3 * rs.standard_normal(int(0.8 * n) - int(0.7 * n))
        x *= 0.3
        xs.append(x.astype(np.float32))
        ys.append((x + rs.standard_normal(n) * np.sqrt(np.mean(x ** 2) / 10 ** 0.5)).astype(np.float32))
    return np.stack(xs), np.stack(ys)


def event_time(fn):
    """Seconds per call from HIP events on the current stream: warm up, size a window to MIN_WINDOW_S, the median of WINDOWS windows."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(MIN_WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    times = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return dict(us=statistics.median(times) * 1e6, us_min=min(times) * 1e6, us_max=max(times) * 1e6, calls_per_window=reps)


def step(name):
    import numpy as np
    rec = dict(step=name, clips=B, seconds_per_clip=SECONDS, sample_rate=SR, windows=WINDOWS)
    if name == "numpy":
        from tests.helpers import stoi_ref as R
        x, y = clips(SECONDS * R.RATE, R.RATE, 1)
        best = {}
        for ext in (False, True):
            ts = []
            for _ in range(3):
                t = time.perf_counter()
                R.stoi64(x[0], y[0], extended=ext)
                ts.append(time.perf_counter() - t)
            best["estoi" if ext else "stoi"] = min(ts)
        rec.update(clips=1, numpy_seconds_per_clip=best, cpus=os.cpu_count())
    else:
        import torch
        from neural_sound_generation_amd import audio as Au
        if not torch.cuda.is_available():
            raise SystemExit("stoi_timing: needs a GPU (cuda:0)")
        dev = torch.device("cuda:0")
        x, y = (torch.from_numpy(a).to(dev) for a in clips(SECONDS * SR, SR, B))
        if name == "resample":
            rec["resample_both"] = event_time(lambda: (Au.resample(x, SR, Au.STOI_RATE), Au.resample(y, SR, Au.STOI_RATE)))
        elif name == "stoi":
            x10, y10 = Au.resample(x, SR, Au.STOI_RATE)[0], Au.resample(y, SR, Au.STOI_RATE)[0]
            env, kept, _, _ = Au.stoi_envelopes(x10, y10)
            rec["frames"], rec["kept_mean"] = int(env.shape[2]), float(kept.double().mean())
            rec["envelopes"] = event_time(lambda: Au.stoi_envelopes(x10, y10))
            rec["score_stoi"] = event_time(lambda: Au.stoi_score(env, kept, False))
            rec["score_estoi"] = event_time(lambda: Au.stoi_score(env, kept, True))
            rec["whole_stoi"] = event_time(lambda: Au.stoi(x, y, SR))
            rec["whole_estoi"] = event_time(lambda: Au.stoi(x, y, SR, extended=True))
            rec["mean_stoi"] = float(Au.stoi(x, y, SR)[0].mean())
            rec["mean_estoi"] = float(Au.stoi(x, y, SR, extended=True)[0].mean())
        elif name == "spectral_convergence":
            T = 1 + SECONDS * SR // 256
            yy = x[:, :256 * (T - 1)].contiguous()
            S = Au.stft(yy, 1024, 256).abs().contiguous()
            rec["frames"] = T
            rec["spectral_convergence"] = event_time(lambda: Au.spectral_convergence(yy, S, 1024, 256))
        else:
            raise SystemExit(f"stoi_timing: unknown step {name!r}")
    print(json.dumps(rec), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rec, fh)


if __name__ == "__main__":
    if "--step" in sys.argv:
        step(sys.argv[sys.argv.index("--step") + 1])
    else:
        driver()
