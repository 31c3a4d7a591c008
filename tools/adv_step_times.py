"""What FGM adversarial training (--adv_epsilon) costs per optimizer step, timed by the driver's own loop as
tools/rdrop_step_times.py does it: run_multimodal_fcmf.py in synthetic mode at the FCMF-base geometry (randomly initialised text
encoder of BASE_CFG, bf16, micro-batch 64), each configuration in a fresh child process:

    plain      one pass per optimizer step
    two_pass   two plain passes per optimizer step (--train_batch_size 128 --gradient_accumulation_steps 2): the yardstick
    adv        a clean and an adversarial pass per optimizer step (--adv_epsilon 0.5)

The driver logs the loss of every 10th (micro-)step through `loss.item()`, a device synchronise; the time is the host clock
between the second and the last such line.  --pool N (default 4) draws N synthetic batches and hands them out in turn (drawing one
per step on the host hides the device's step).  Prints one JSON line per configuration (and appends them to --out when given).

    python tools/adv_step_times.py [--steps 61] [--pool 4] [--out FILE]
"""
import argparse
import json
import logging
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multimodal-aspect-category-sentiment-analysis_amd")
sys.path.insert(0, PKG)

MICRO = 64
CONFIGS = [("plain", 1, 0.0), ("two_pass", 2, 0.0), ("adv", 1, 0.5)]      # name, micro-steps per optimizer step, epsilon


class _Clock(logging.Handler):
    def __init__(self):
        super().__init__()
        self.marks = []

    def emit(self, record):
        m = re.search(r"step (\d+) loss (\S+)", record.getMessage())
        if m:
            self.marks.append((int(m.group(1)), time.perf_counter(), float(m.group(2))))


def child(name, accum, epsilon, steps, hf, pool):
    import torch
    import synthetic_data as synth
    if pool > 0:
        draw, drawn = synth.synth_batch, {}

        def pooled(*args, seed=42, **kw):
            if seed % pool not in drawn:
                drawn[seed % pool] = draw(*args, seed=seed, **kw)
            return drawn[seed % pool]
        synth.synth_batch = pooled
    out = tempfile.mkdtemp(prefix="adv_times_")
    clock = _Clock()
    import run_multimodal_fcmf as drv
    logging.getLogger("fcmf").addHandler(clock)
    drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--do_train", "--bf16", "--train_batch_size", str(MICRO * accum),
              "--gradient_accumulation_steps", str(accum), "--synthetic_steps", str(steps), "--num_train_epochs", "1", "--seed", "1",
              "--num_imgs", "7", "--num_rois", "4", "--max_seq_length", "128", "--adv_epsilon", str(epsilon)])
    torch.cuda.synchronize()
    shutil.rmtree(out, ignore_errors=True)     # (the checkpoints of a base-size run: not what is measured)
    (s0, t0, _), (s1, t1, last) = clock.marks[1], clock.marks[-1]
    per_micro = (t1 - t0) * 1e3 / (s1 - s0)
    print(json.dumps({"bench": "adv_step", "config": name, "micro_batch": MICRO, "micro_steps_per_optimizer_step": accum,
                      "adv_epsilon": epsilon, "batch_pool": pool, "micro_steps_timed": s1 - s0,
                      "ms_per_optimizer_step": round(per_micro * accum, 2), "last_loss": last,
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=61)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        name, accum, epsilon, hf = a.child
        return child(name, int(accum), float(epsilon), a.steps, hf, a.pool)
    import synthetic_data as synth
    from fcmf_framework.roberta import RobertaConfig, RobertaModel
    hf = tempfile.mkdtemp(prefix="hf_base_")
    RobertaModel(RobertaConfig(**synth.BASE_CFG)).save_pretrained(hf)
    for name, accum, epsilon in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--pool", str(a.pool), "--child", name,
                            str(accum), str(epsilon), hf], stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode != 0:                  # (a configuration that died: nothing more is started on the device)
            sys.exit(f"{name}: exit status {r.returncode}")
        line = [x for x in r.stdout.splitlines() if x.startswith('{"bench"')][-1]
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    shutil.rmtree(hf, ignore_errors=True)


if __name__ == "__main__":
    main()
