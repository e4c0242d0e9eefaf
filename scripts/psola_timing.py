"""Timing of the PSOLA pitch shifter and of what it adds to training, each figure the median over windows of HIP-event times on
the launch stream (every call warmed up; a window is a run of whole calls between two events; min and max of the windows beside
it are the run's own spread):
  * psola: 64 clips of 10 s at 22 050 Hz -- ops.pitch_marks (the chain over the analysis marks), ops.psola (the chain over the
    synthesis marks and the overlap-add), audio.pitch_shift_psola (both, with its uploads), audio.pitch_shift (tempo + resample)
    on the same batch in the same run, audio.f0 beside them, and the numpy restatement (tests/helpers/psola_ref.py) of one clip;
  * perturb: what train.train_conditioned(pitch_perturb=) adds per batch at BASELINE configs[2]'s batch (128 clips of 1024 mel
    frames = 262 144 samples): audio.perturb_pitch (tracking + PSOLA) and audio.melspectrogram, beside audio.f0 alone;
  * step: the fused bf16 step at configs[2]'s widths with target=c2 against the same step without a target, alternating.
Without --step this is the driver: every step is a process of its own under `timeout -k 10 <seconds>`, the steps chained so that
the first failure ends the run; --json PATH collects the steps' records.  There is no fallback: without a GPU the steps fail.
    python scripts/psola_timing.py [--json profiles/psola_timing.json]"""
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
STEPS = (("psola", 240), ("perturb", 240), ("step", 240))     # (step, its time limit in seconds)
WINDOWS, MIN_WINDOW_S = 9, 0.1


def driver():
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    scratch = tempfile.mkdtemp(prefix="psola_timing_")
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
        raise SystemExit(f"psola_timing: a step failed (exit status {rc}); nothing more was started")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(records, fh, indent=1)


def event_time(fn):
    """Milliseconds per call from HIP events on the current stream: warm up, size a window to MIN_WINDOW_S, the median of WINDOWS windows."""
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
        times.append(a.elapsed_time(b) / reps)
    return dict(ms=statistics.median(times), ms_min=min(times), ms_max=max(times), calls_per_window=reps)


def glides(B, n, sr=22050):
    """B harmonic tones of n samples whose pitch wanders +-20 % about 100 + 2 b Hz."""
    import numpy as np
    t = np.arange(n, dtype=np.float64)
    return np.stack([0.3 * sum(0.6 ** h * np.sin(h * 2 * np.pi * np.cumsum((100.0 + 2 * b) * (1.0 + 0.2 * np.sin(2 * np.pi * t / sr)) / sr))
                               for h in range(1, 7)) for b in range(B)]).astype(np.float32)


def step(name):
    import numpy as np
    import torch
    from neural_sound_generation_amd import audio as Au, models as M, ops
    from neural_sound_generation_amd.train import FusedTrainStep
    if not torch.cuda.is_available():
        raise SystemExit("psola_timing: needs a GPU (cuda:0)")
    dev = torch.device("cuda:0")
    rec = dict(step=name, windows=WINDOWS)
    gen = torch.Generator(device=dev).manual_seed(3)
    SR, HOP = 22050, 256
    if name == "psola":
        from tests.helpers import psola_ref as R
        B, n = 64, 10 * SR
        host = glides(B, n)
        wav = torch.from_numpy(host).to(dev)
        f0, _ = Au.f0(wav)
        P_u, P_min, P_max = Au.psola_periods(SR)
        P = (HOP, float(SR), P_u, P_min, P_max, Au.PSOLA_ALPHA)
        f_out = (f0 * 1.25).contiguous()
        marks, n_marks = ops.pitch_marks(wav, f0, *P)
        _, _, _, n_syn = ops.psola(wav, f0, f_out, marks, n_marks, *P)
        rec.update(clips=B, samples=n, frames=int(f0.shape[1]), voiced_share=float((f0 > 0).double().mean()),
                   marks_per_clip=float(n_marks.double().mean()), syn_marks_per_clip=float(n_syn.double().mean()))
        rec["audio_f0"] = event_time(lambda: Au.f0(wav))
        rec["pitch_marks_chain"] = event_time(lambda: ops.pitch_marks(wav, f0, *P))
        rec["psola_syn_chain_and_overlap_add"] = event_time(lambda: ops.psola(wav, f0, f_out, marks, n_marks, *P))
        rec["pitch_shift_psola"] = event_time(lambda: Au.pitch_shift_psola(wav, f0, ratio=1.25))
        rec["pitch_shift_tempo_resample_5_4"] = event_time(lambda: Au.pitch_shift(wav, 5, 4))
        rec["pitch_marks_chain_again"] = event_time(lambda: ops.pitch_marks(wav, f0, *P))
        one = ops.pitch_marks(wav[:1].contiguous(), f0[:1].contiguous(), *P)
        rec["pitch_marks_chain_one_clip"] = event_time(lambda: ops.pitch_marks(wav[:1], f0[:1], *P))
        f_h, fo_h = f0[0].cpu().numpy(), f_out[0].cpu().numpy()
        t = time.perf_counter()
        ref = R.psola_ref(host[0], n, f_h, fo_h, HOP, SR, P_u, P_min, P_max)
        rec["numpy_restatement_one_clip_s"] = time.perf_counter() - t
        assert ref["marks"] == one[0][0, :int(one[1][0])].tolist()
    elif name == "perturb":
        B, T = 128, 1024
        wav = torch.from_numpy(glides(8, T * HOP)).to(dev).repeat(B // 8, 1).contiguous()
        g = torch.Generator().manual_seed(1)
        rec.update(clips=B, samples=T * HOP)
        rec["audio_f0"] = event_time(lambda: Au.f0(wav))
        rec["melspectrogram"] = event_time(lambda: Au.melspectrogram(wav))
        rec["perturb_pitch_tracking_and_psola"] = event_time(lambda: Au.perturb_pitch(wav, None, g))
        rec["perturb_pitch_then_melspectrogram"] = event_time(lambda: Au.melspectrogram(Au.perturb_pitch(wav, None, g)[0]))
        rec["audio_f0_again"] = event_time(lambda: Au.f0(wav))
    elif name == "step":
        B, T, D, K, S, NB = 128, 1024, 128, 512, 7, 32
        c = torch.rand(B, 1, 80, T, device=dev, generator=gen)
        c2 = torch.rand(B, 1, 80, T, device=dev, generator=gen)
        g = torch.randint(0, S, (B,), device=dev, generator=gen)
        bins = torch.randint(0, NB + 1, (B, T // 4), device=dev, generator=gen)
        rec.update(B=B, T=T, D=D, K=K, n_speakers=S, n_f0_bins=NB)
        torch.manual_seed(1)
        st = FusedTrainStep(M.VQVAE(1, D, K, n_speakers=S, n_f0_bins=NB, compute_dtype=torch.bfloat16).to(dev).train())
        rec["step_without_target"] = event_time(lambda: st.step(c, g, bins))
        rec["step_with_target"] = event_time(lambda: st.step(c2, g, bins, target=c))
        rec["step_without_target_again"] = event_time(lambda: st.step(c, g, bins))
        rec["step_with_target_again"] = event_time(lambda: st.step(c2, g, bins, target=c))
    else:
        raise SystemExit(f"psola_timing: unknown step {name!r}")
    print(json.dumps(rec), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(rec, fh)


if __name__ == "__main__":
    if "--step" in sys.argv:
        step(sys.argv[sys.argv.index("--step") + 1])
    else:
        driver()
