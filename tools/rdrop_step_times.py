"""What R-Drop costs per training step, timed by the drivers' own loop: run_multimodal_fcmf.py and
run_pretraining_fcmf.py in synthetic mode at the FCMF-base geometry (randomly initialised text encoder of BASE_CFG, bf16), each
configuration in a fresh child process.  The drivers log the loss of every 10th step through `loss.item()`, a device
synchronise; a step's time is the host clock between the second and the last such line over the steps between them (the first
interval holds the warm-up).  The synthetic batches are drawn on the host, one per step, which at this geometry takes ~6 ms per
review and hides the device's step entirely; --pool N (default 4) therefore draws N batches and hands them out in turn, --pool 0
leaves the generator as it is.  Prints one JSON line per configuration (and appends them to --out when given).

    python tools/rdrop_step_times.py [--steps 61] [--pool 4] [--out FILE]
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

CONFIGS = [("fcmf", 64, 0.0), ("fcmf", 32, 1.0), ("fcmf", 64, 1.0), ("fcmf", 128, 0.0), ("iaog", 64, 0.0), ("iaog", 64, 1.0)]


class _Clock(logging.Handler):
    def __init__(self):
        super().__init__()
        self.marks = []

    def emit(self, record):
        m = re.search(r"step (\d+) loss (\S+)", record.getMessage())
        if m:
            self.marks.append((int(m.group(1)), time.perf_counter(), float(m.group(2))))


def child(workload, batch, alpha, steps, hf, pool):
    import torch
    import synthetic_data as synth
    if pool > 0:
        draw, drawn = synth.synth_batch, {}

        def pooled(*args, seed=42, **kw):
            if seed % pool not in drawn:
                drawn[seed % pool] = draw(*args, seed=seed, **kw)
            return drawn[seed % pool]
        synth.synth_batch = pooled
    out = tempfile.mkdtemp(prefix="rdrop_times_")
    clock = _Clock()
    if workload == "fcmf":
        import run_multimodal_fcmf as drv
        logging.getLogger("fcmf").addHandler(clock)
        argv = ["--num_imgs", "7", "--num_rois", "4", "--max_seq_length", "128", "--gradient_accumulation_steps", "1"]
    else:
        import run_pretraining_fcmf as drv
        logging.getLogger("iaog").addHandler(clock)
        argv = ["--num_imgs", "7", "--num_rois", "4", "--max_seq_length", "128", "--synthetic_dec_len", "12"]
    drv.main(["--output_dir", out, "--pretrained_hf_model", hf, "--do_train", "--bf16", "--train_batch_size", str(batch),
              "--synthetic_steps", str(steps), "--num_train_epochs", "1", "--seed", "1", "--rdrop_alpha", str(alpha)] + argv)
    torch.cuda.synchronize()
    shutil.rmtree(out, ignore_errors=True)     # (the checkpoints of a base-size run: not what is measured)
    (s0, t0, _), (s1, t1, last) = clock.marks[1], clock.marks[-1]
    print(json.dumps({"bench": "rdrop_step", "workload": workload, "batch": batch, "rdrop_alpha": alpha, "batch_pool": pool, "steps_timed": s1 - s0,
                      "ms_per_step": round((t1 - t0) * 1e3 / (s1 - s0), 2), "last_loss": last,
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=61)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        workload, batch, alpha, hf = a.child
        return child(workload, int(batch), float(alpha), a.steps, hf, a.pool)
    import synthetic_data as synth
    from fcmf_framework.roberta import RobertaConfig, RobertaModel
    hf = tempfile.mkdtemp(prefix="hf_base_")
    RobertaModel(RobertaConfig(**synth.BASE_CFG)).save_pretrained(hf)
    for workload, batch, alpha in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--pool", str(a.pool), "--child", workload, str(batch), str(alpha), hf],
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode != 0:                  # (a configuration that died: nothing more is started on the device)
            sys.exit(f"{workload} B={batch} alpha={alpha}: exit status {r.returncode}")
        line = [x for x in r.stdout.splitlines() if x.startswith('{"bench"')][-1]
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    shutil.rmtree(hf, ignore_errors=True)


if __name__ == "__main__":
    main()
