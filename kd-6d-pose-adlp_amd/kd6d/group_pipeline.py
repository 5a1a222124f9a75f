"""Which batch sits where in the grouped teacher pass, and what a call issues: the one statement of the rules (DESIGN.md
section 5).  Host logic only -- `GroupedTeacherKDStep` (kd6d/graph.py) does the device work behind the five calls below,
`tests/test_grouped_pipeline_cpu.py` puts a ledger in its place.

Three blocks of `group` batches each:
    LOAD     being filled, one batch per call (`n_loaded` of its slots hold one);
    PASS     the teacher's input (`p_valid` batches) and, once its last segment has run, its cells; `t_pos` is the next
             of the pass's `group` segments to issue;
    CURRENT  what the student trains on: `c_valid` batches that carry teacher cells, `c_pos` the next slot to train on.

Call k = m * group + s of `feed()`
    loads batch k into slot s of LOAD,
    issues teacher segment s over PASS = the batches of period m - 1 (never more than segment s before student step s:
    one segment beside every student step is the pacing the step time depends on),
    issues student step s on slot s of CURRENT = batch k - 2 * group, after the student's graphs are known to exist,
and the last call of a period issues whatever segments of the pass are left and ROTATES: CURRENT <- PASS <- LOAD.  A
rotation never happens before the last segment, so the student never trains on a block the teacher has not finished.
Every batch gets exactly one teacher pass and one student step, in the order fed; a call returns the student step's
result for batch k - 2 * group, None for the first 2 * group calls.

`flush()` trains on ONE pending batch without taking a new one (None when nothing is pending): while CURRENT has nothing
trainable it finishes the teacher on PASS and rotates, a partly filled LOAD block included.  Once a drain has begun,
`feed()` refuses new batches until it is complete; the next `feed()` then starts a new pipeline.

The interface `dev` (every call is issued in the order given above):
    load_slot(s, *batch)               put a batch into slot s of LOAD
    replay_teacher_segment(i)          segment i of the pass over PASS
    ensure_captured()                  the student's graphs exist (called before a step's teacher segment goes out)
    replay_student(s) -> result        the student step on slot s of CURRENT
    rotate_blocks(pass_valid, n_loaded)  CURRENT <- PASS if pass_valid, PASS <- LOAD if n_loaded (a partial LOAD block
                                       has its free slots filled first)
"""


class GroupPipeline:
    def __init__(self, group, dev):
        self.group, self.dev = int(group), dev
        self.n_loaded = 0                 # batches in the load block
        self.p_valid = 0                  # batches of the pass block (the teacher's input)
        self.t_pos = 0                    # next teacher segment of the pass block
        self.c_valid = 0                  # batches of the current block (they carry teacher cells)
        self.c_pos = 0                    # next slot of the current block to train on
        self.draining = False
        self.teacher_passes = 0           # completed group passes

    @property
    def pending_steps(self):
        """Batches fed that have not had their student step yet."""
        return (self.c_valid - self.c_pos) + self.p_valid + self.n_loaded

    def _load(self, batch):
        assert self.n_loaded < self.group
        self.dev.load_slot(self.n_loaded, *batch)
        self.n_loaded += 1

    def _rotate(self):
        """Period end: CURRENT <- PASS <- LOAD.  The caller has issued every teacher segment of the pass block."""
        self.dev.rotate_blocks(bool(self.p_valid), self.n_loaded)
        self.c_valid, self.p_valid, self.n_loaded = self.p_valid, self.n_loaded, 0
        self.c_pos = self.t_pos = 0

    def _teacher_segments(self, upto):
        """Issue the pass block's segments t_pos .. upto - 1."""
        while self.p_valid and self.t_pos < upto:
            self.dev.replay_teacher_segment(self.t_pos)
            self.t_pos += 1
            if self.t_pos == self.group:
                self.teacher_passes += 1

    def _tick(self, drain):
        T = self.group
        if drain:
            while self.c_pos >= self.c_valid:      # nothing trainable: finish the teacher on the pass block, rotate
                self._teacher_segments(T)
                self._rotate()
        out = None
        if self.c_pos < self.c_valid:
            s = self.c_pos
            self.dev.ensure_captured()             # (before this step's teacher segment goes out)
            self._teacher_segments(s + 1)          # segment s beside student step s
            out = self.dev.replay_student(s)
            self.c_pos += 1
        if not drain and self.n_loaded == T:       # period end
            self._teacher_segments(T)
            self._rotate()
        return out

    def feed(self, *batch):
        """One batch in; the result of the student step on batch k - 2 * group, None while the pipeline fills."""
        if self.draining:
            if self.pending_steps > 0:
                raise RuntimeError("GroupedTeacherKDStep: flush() the %d pending batches before feeding new ones"
                                   % self.pending_steps)
            self.draining = False
        self._load(batch)
        return self._tick(False)

    def flush(self):
        if self.pending_steps == 0:
            return None
        self.draining = True
        return self._tick(True)

    def prime(self, *batch):
        """Walk a sample batch through all three blocks, so that every graph gets recorded, and leave the pipeline as
        empty as a fresh one (GroupedTeacherKDStep.prepare)."""
        if self.pending_steps:
            raise RuntimeError("GroupedTeacherKDStep.prepare(): call it before the first batch is fed")
        for _ in range(self.group):
            self._load(batch)
        self._rotate()                          # PASS <- LOAD
        self._teacher_segments(self.group)      # records the teacher's graphs (and runs them once: cells of the sample)
        self._rotate()                          # CURRENT <- PASS
        self.dev.ensure_captured()              # the student's graphs; snapshot / restore around their warm-up steps
        self.n_loaded = self.p_valid = self.t_pos = self.c_valid = self.c_pos = 0
        self.teacher_passes = 0
