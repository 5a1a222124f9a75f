"""Does the engine learn a pose from rendered frames?  Run on the GPU box.

    python tools/render_learnability.py [--iters 3000] [--val_freq 500] [--frames 2048] [--valid_frames 128]
                                        [--stages student,teacher,kd] [--out profiles/render_learnability]

Three stages on --frame_source render --render_meshes surrogate, one class (class 0):
  student  darknet_tiny_h, --kd_weight 0.                        (the teacher is built but its term has no weight)
  teacher  darknet53, --kd_weight 0.: the teacher recipe, trained the same way; its final.pth feeds the third stage
  kd       darknet_tiny_h, --kd_weight 5., --weight_file_t the teacher just trained
A stage is two train_kd.py child processes, each under its own time limit: `--max_iters 0`, which validates the UNTRAINED
network on the rendered valid list (a fixed seed, never refreshed: step 0, "the start"), then the training run, which
validates every --val_freq steps and at the end.  What is recorded comes from the run's scalar log (scalars.jsonl in its
working directory, what train_kd.py's ScalarWriter writes when tensorboardX is not importable): ADI/all_class and
REP/all_class of every validation, and the unweighted training/loss_cls, loss_reg, loss_kd (logged every 10 steps; kept
here at the first log, every 100 steps and the last).

THE FIRST CHILD THAT DOES NOT END WITH STATUS 0 -- a failure, a GPU fault or abort, or its time limit -- ENDS THE TOOL:
what was recorded so far is written, nothing more is started on the GPU, and the exit status is 1.
Nothing is asserted about the figures: the record goes into profiles/render_frames.md whatever it says.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_scalars(wd):
    """-> (losses [{step, loss_cls, loss_reg, loss_kd}], valid [{step, ADI.., REP..}]) of a working directory's scalar log."""
    path = os.path.join(wd, "scalars.jsonl")
    if not os.path.exists(path):
        return None, None
    losses, valid = {}, {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            tag, step = r["tag"], int(r["step"])
            if tag in ("training/loss_cls", "training/loss_reg", "training/loss_kd"):
                losses.setdefault(step, {"step": step})[tag.split("/")[1]] = round(r["value"], 5)
            elif tag.startswith(("ADI/all_class/", "REP/all_class/")):
                valid.setdefault(step, {"step": step})[tag.split("/")[2]] = round(r["value"], 3)
    ls = [losses[s] for s in sorted(losses)]
    keep = [x for i, x in enumerate(ls) if i == 0 or i == len(ls) - 1 or x["step"] % 100 == 0]
    return keep, [valid[s] for s in sorted(valid)]


def run_child(args, wd, iters, frames, extra, limit):
    """One train_kd.py process -> (ok, record).  ok is False for any end but exit status 0."""
    cmd = [sys.executable, os.path.join(HERE, "train_kd.py"), "--config_file", os.path.join(HERE, "configs", "ape.yaml"),
           "--config_file_t", os.path.join(HERE, "configs", "ape.yaml"), "--working_dir", wd, "--max_iters", str(iters),
           "--val_freq", str(args.val_freq), "--frame_source", "render", "--render_meshes", "surrogate",
           "--render_frames", str(frames), "--render_valid_frames", str(args.valid_frames), "--render_instances", "1",
           "--render_refresh", "epoch", "--skip_teacher_eval", "--pnp_solver", "device", "--eval_scorer", "device",
           "--num_workers", "0"] + extra
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=HERE)
    except subprocess.TimeoutExpired:
        return False, {"max_iters": iters, "time_limit_s": limit}
    rec = {"max_iters": iters, "returncode": r.returncode, "seconds": round(time.time() - t0, 1)}
    if r.returncode != 0:
        rec["tail"] = r.stdout[-1500:] + r.stderr[-1500:]
        return False, rec
    rec["losses"], rec["valid"] = read_scalars(wd)
    if rec["valid"] is None:
        rec["note"] = "no scalars.jsonl in the working directory (tensorboardX took the scalars): nothing to read"
    return True, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--val_freq", type=int, default=500)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--valid_frames", type=int, default=128)
    ap.add_argument("--stages", type=str, default="student,teacher,kd")
    ap.add_argument("--limit", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--work", type=str, default="outputs/render_learnability")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    work = os.path.abspath(a.work)
    teacher_pth = os.path.join(work, "teacher", "final.pth")
    extra = {"student": ["--backbone", "darknet_tiny_h", "--kd_weight", "0."],
             "teacher": ["--backbone", "darknet53", "--kd_weight", "0."],
             "kd": ["--backbone", "darknet_tiny_h", "--kd_weight", "5.", "--weight_file_t", teacher_pth]}
    res, ok = [], True
    for name in a.stages.split(","):
        if name == "kd" and not os.path.exists(teacher_pth):
            res.append({"stage": "kd", "skipped": "no trained teacher (stage teacher has not run)"})
            continue
        stage = {"stage": name, "flags": " ".join(extra[name][:4])}
        res.append(stage)
        # the untrained network on the valid list (16 training frames: the list is built but no step is taken), then the run
        for key, iters, frames in (("start", 0, 16), ("run", a.iters, a.frames)):
            ok, rec = run_child(a, os.path.join(work, name + ("_start" if key == "start" else "")), iters, frames,
                                extra[name], a.limit)
            stage[key] = rec
            if not ok:
                break
            for v in rec.get("valid") or []:
                print("%-8s %-5s valid @ %5d: %s" % (name, key, v["step"], {k: x for k, x in v.items() if k != "step"}))
            if key == "run" and rec.get("losses"):
                print("%-8s %5.0f s  losses %s -> %s" % (name, rec["seconds"], rec["losses"][0], rec["losses"][-1]))
        if not ok:
            print("%-8s did not end with status 0: %s\nstopping here: nothing more is started on the GPU"
                  % (name, stage[key].get("tail", "time limit of %d s" % a.limit)))
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
