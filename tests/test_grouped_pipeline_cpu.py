"""CPU: the bookkeeping of kd6d.graph.GroupedTeacherKDStep -- kd6d.group_pipeline.GroupPipeline: which batch sits in which
block, which teacher segment and which student step a call issues, what flush() drains -- driven directly, with a ledger
as the interface the step class implements on the device.  The properties the GPU
parity tests rely on, for every group size and every point at which feeding stops:
  * every batch fed is trained on exactly once, in the order it was fed;
  * when a batch is trained on, the teacher has run ALL its segments over the block that held it, after the batch (and
    its whole period) had been loaded -- never over a half-loaded block;
  * in steady state every call issues exactly one teacher segment and one student step (the pacing the step time
    depends on), and a period's last call rotates the blocks;
  * flush() drains one batch per call, returns None when the pipeline is empty, and a later call starts a new pipeline."""
import itertools

import pytest

from kd6d.group_pipeline import GroupPipeline


class Ledger(GroupPipeline):
    """The real pipeline, with this ledger as its device interface."""

    def __init__(self, group):
        super().__init__(group, self)
        self.load = [None] * group          # batch ids per slot
        self.pas = [None] * group
        self.cur = [None] * group
        self.pas_segments = set()           # teacher segments run over the pass block since it was filled
        self.cur_segments = set()           # ... that the current block's cells come from
        self.trained, self.events = [], []
        self.captured = 0                   # ensure_captured() calls

    __call__ = GroupPipeline.feed

    @property
    def pending(self):                      # as both step classes derive it
        return self.pending_steps > 0

    def load_slot(self, s, images, tgt):
        self.load[s] = images
        self.events.append(("load", s))

    def rotate_blocks(self, pass_valid, n_loaded):
        if 0 < n_loaded < self.group:
            for s in range(n_loaded, self.group):
                self.load[s] = ("filler", self.load[0])
        if pass_valid:
            self.cur, self.cur_segments = list(self.pas), set(self.pas_segments)
        if n_loaded:
            self.pas, self.pas_segments = list(self.load), set()
        self.events.append(("rotate",))

    def replay_teacher_segment(self, i):
        assert i == len(self.pas_segments), "segments run in order, each once per block"
        self.pas_segments.add(i)
        self.events.append(("teacher", i))

    def ensure_captured(self):
        self.captured += 1

    def replay_student(self, s):
        assert self.cur_segments == set(range(self.group)), "student step on a block the teacher has not finished"
        b = self.cur[s]
        assert b is not None and not (isinstance(b, tuple) and b[0] == "filler")
        self.trained.append(b)
        self.events.append(("student", s))
        return {"batch": b}


@pytest.mark.parametrize("group", [2, 3, 4])
def test_every_batch_trained_once_in_order(group):
    for n in range(0, 4 * group + 2):
        gs = Ledger(group)
        outs = [gs(i, None) for i in range(n)]
        assert all((o is None) == (i < 2 * group) for i, o in enumerate(outs))
        assert [o["batch"] for o in outs if o is not None] == list(range(max(0, n - 2 * group)))
        assert gs.pending_steps == n - len(gs.trained) == min(n, 2 * group)
        drained = []
        while True:
            o = gs.flush()
            if o is None:
                break
            drained.append(o["batch"])
        assert gs.trained == list(range(n)), (group, n, gs.trained)
        assert gs.pending_steps == 0 and not gs.pending and gs.flush() is None
        # a later call starts a new pipeline
        assert gs("again", None) is None and gs.pending_steps == 1


@pytest.mark.parametrize("group", [2, 3, 5])
def test_steady_state_issues_one_segment_and_one_step_per_call(group):
    gs = Ledger(group)
    for i in range(2 * group):
        gs(i, None)
    gs.events.clear()
    for k in range(3 * group):
        mark = len(gs.events)
        gs(2 * group + k, None)
        ev = gs.events[mark:]
        s = k % group
        want = [("load", s), ("teacher", s), ("student", s)] + ([("rotate",)] if s == group - 1 else [])
        assert ev == want, (k, ev)
    assert gs.teacher_passes == 3 + 1          # one during the filling periods, one per steady period


def test_feeding_a_partly_drained_pipeline_is_refused():
    gs = Ledger(2)
    for i in range(6):
        gs(i, None)
    assert gs.flush() is not None and gs.pending_steps == 3
    with pytest.raises(RuntimeError, match="flush"):
        gs(99, None)
    while gs.flush() is not None:
        pass
    assert gs.trained == list(range(6))


@pytest.mark.parametrize("group", [2, 3, 4])
def test_prime_records_everything_and_leaves_a_fresh_pipeline(group):
    """GroupedTeacherKDStep.prepare(): the sample goes through all three blocks -- `group` loads, PASS <- LOAD, every
    teacher segment, CURRENT <- PASS, the student's graphs -- and afterwards nothing tells the pipeline from a new one."""
    gs = Ledger(group)
    gs.prime("sample", None)
    assert gs.events == ([("load", s) for s in range(group)] + [("rotate",)]
                         + [("teacher", i) for i in range(group)] + [("rotate",)])
    assert gs.captured == 1 and gs.trained == []
    assert (gs.n_loaded, gs.p_valid, gs.t_pos, gs.c_valid, gs.c_pos, gs.teacher_passes) == (0, 0, 0, 0, 0, 0)
    assert not gs.draining and gs.pending_steps == 0 and gs.flush() is None
    fresh = Ledger(group)
    for i in range(2 * group):
        mark = len(gs.events), len(fresh.events)
        assert gs(i, None) is None and fresh(i, None) is None
        assert gs.events[mark[0]:] == fresh.events[mark[1]:]
    assert gs(2 * group, None) == {"batch": 0}             # ... and the sample is never trained on
    gs2 = Ledger(group)
    gs2(0, None)
    with pytest.raises(RuntimeError, match="before the first batch"):
        gs2.prime("sample", None)


def test_group_of_one_is_the_plain_pipeline():
    from kd6d.graph import GroupedTeacherKDStep
    with pytest.raises(ValueError):
        GroupedTeacherKDStep(None, None, None, group=1)
