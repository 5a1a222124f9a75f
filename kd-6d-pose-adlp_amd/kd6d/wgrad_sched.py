"""Where and when the reverse sweep issues a layer's weight gradient: the one statement of the rules.

A weight gradient feeds nothing in the sweep, so it may leave the chain's stream and overlap the dgrad / normalisation
chain (both under-fill 256 CUs at these layer sizes).  `WgradSchedule.submit` takes the first of four ways that applies
to the layer:

  1. GROUP   while the sweep is inside the head (begin() ... close_group_section()), in bf16, for a geometry the grouped
             kernel takes (ops.wgrad_group_supported): collected into the network's ops.WgradGroup.  The FPN output
             convolutions join it through try_group() once d_head_in is complete.  The group goes out as one launch
             pair at flush_group("head_end") or flush_group("fpn_end"), whichever PoseNet.wgrad_group_flush names.
  2. LIST    a side stream exists, option wgrad.list > 1, and the sweep is not in its tail: the call waits in `pending`;
             when the option's value is reached flush_list() forks ONCE (one wait_stream, one side stream) for one
             ops.conv2d_wgrad_list.  A pending call takes no stream until its flush.
  3. FORK    a side stream exists: one fork for this layer alone.
  4. IN LINE no side stream: on the chain's stream, sized for the whole device (budget 0).

Every fork -- a list, a single layer, the group -- takes the NEXT of the side streams, round-robin.  The tail: from the
tape index tail_start() gives, the last WGRAD_LIST_TAIL_BLOCKS blocks of the backbone sweep, enter_tail() flushes and
every layer forks alone again (a list launched behind the last chain kernel would run with nothing beside it).  The
caller flushes the list before its grad_hook (installed by kd6d.libs.distributed.overlapped_exchange, which waits on
streams() there), and finish() flushes what is left and joins every side stream once.

The per-layer call is built when the layer is reached (its slab, Conv.wgrad_slab, is taken then, not at the flush): a
pending call reads x and dy later than the sweep reached the layer, which the sweep never writes again.

The knobs are plain attributes of the PoseNet (side_stream, side_streams, wgrad_cu_budget, use_wgrad_group,
wgrad_group_wgs, wgrad_group_flush), read when needed; the launchers are the `ops` namespace the engine hands over, so a
recording stand-in put in its place sees every launch.  Nothing here touches the device at import time."""
import torch


class WgradSchedule:
    WGRAD_LIST_TAIL_BLOCKS = 2      # blocks at the end of the backbone sweep whose weight gradients fork per layer

    def __init__(self, net, ops):
        self.net, self.ops = net, ops
        self.rr = 0                 # index of the side stream the last fork took
        self.pending = []           # per-layer calls waiting for their list launch
        self.tail = False           # the sweep is inside its last blocks
        self.group = None           # ops.WgradGroup, created by the first begin() that wants one
        self.grouping = False       # the sweep is inside the section whose weight gradients the group collects

    # ---- streams and sizes -------------------------------------------------------------------
    def streams(self):
        """The side streams, possibly none."""
        net = self.net
        return list(net.side_streams or ([net.side_stream] if net.side_stream is not None else []))

    def budget(self):
        """CU budget of a per-layer weight-gradient launch (ops.conv2d_wgrad, ops.bn_pool_bwd_wgrad): the share
        wgrad_cu_budget when these launches are forked onto side streams, the whole device (0) when they run on the
        chain's stream.  The one place that decides it: slab sizes and launches agree."""
        return self.net.wgrad_cu_budget if self.streams() else 0

    def list_limit(self):
        """How many per-layer calls are collected before one fork (option wgrad.list); 0: a fork per layer -- no side
        stream to fork onto, the option off, or the end of the sweep."""
        if self.tail or not self.streams():
            return 0
        n = self.ops.get_option("wgrad.list")
        return n if n > 1 else 0

    def _fork(self, launch):
        """launch() on the next side stream, behind what the chain's stream holds so far; in line without one."""
        streams = self.streams()
        if not streams:
            launch()
            return
        self.rr = (self.rr + 1) % len(streams)
        side = streams[self.rr]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()

    # ---- the sweep, in the order PoseNet.backward calls ---------------------------------------------
    def begin(self):
        net = self.net
        if net.use_wgrad_group and net.dtype == torch.bfloat16 and self.group is None:
            self.group = self.ops.WgradGroup(net.wgrad_group_wgs or max(self.ops.device_cu_count() // 2, 1))
        self.grouping = self.group is not None
        self.pending, self.tail = [], False        # (an aborted sweep may have left calls behind)

    def try_group(self, conv, geom, x, dy):
        """Collect the layer into the group if the grouped section is open and the kernel takes it."""
        if not (self.grouping and x.dtype == torch.bfloat16 and self.ops.wgrad_group_supported(geom, x.dtype)):
            return False
        # x and dy are per-layer buffers that stay untouched until the sweep has joined its side streams
        st = self.net.store
        self.group.add(geom, x, dy, st.storage(conv.w, "grads"), None if conv.b is None else st.storage(conv.b, "grads"),
                       flops=conv.flops(geom))
        return True

    def submit(self, conv, geom, x, dy):
        """The layer's weight gradient (+ bias gradient): grouped, listed, forked alone or in line."""
        if self.try_group(conv, geom, x, dy):
            return
        st, budget = self.net.store, self.budget()
        call = dict(flops=conv.flops(geom), dbias=None if conv.b is None else st.acc(conv.b), acc_stride=st.acc_stride,
                    cu_budget=budget)
        slab = conv.wgrad_slab(geom, x.dtype, budget)
        limit = self.list_limit()
        if limit > 1:
            self.pending.append(dict(call, geom=geom, x=x, dy=dy, dw_slab=slab))
            if len(self.pending) >= limit:
                self.flush_list()
        else:
            self._fork(lambda: self.ops.conv2d_wgrad(geom, x, dy, slab, **call))

    def flush_list(self):
        """One fork for the collected per-layer calls (the transposing-family ones side by side inside list launches)."""
        calls = self.pending
        if calls:
            self.pending = []
            self._fork(lambda: self.ops.conv2d_wgrad_list(calls))

    def close_group_section(self):
        """d_head_in is complete and the FPN output convolutions have been offered: layers from here on go per layer."""
        self.grouping = False

    def flush_group(self, at):
        """Launch the group if `at` ("head_end" | "fpn_end") is the point PoseNet.wgrad_group_flush names.  Measured:
        beside the FPN / backbone sweep when a teacher forward shares the device (pipelined steps: 5363-5382 images/s
        against 5107-5135 with the launch behind the FPN sweep); strictly sequential steps launch it behind the FPN
        sweep, beside the backbone sweep's chain of small launches (4836 against 4655).  At the very end of the sweep it
        costs 2-7 % of the step (it then runs with nothing beside it)."""
        want = "fpn_end" if self.net.wgrad_group_flush == "fpn_end" else "head_end"
        if at == want and self.group is not None and len(self.group):
            self._fork(self.group.launch)

    def tail_start(self, tape):
        """Tape index at which the reverse sweep enters its last WGRAD_LIST_TAIL_BLOCKS blocks (each tape record says
        whether it is one: a DarkUnit counts as one, markers and pools as none)."""
        blocks = [i for i, rec in enumerate(tape) if rec.is_block]
        n = min(self.WGRAD_LIST_TAIL_BLOCKS, len(blocks))
        return blocks[n - 1] if n else -1

    def enter_tail(self):
        # the lists collected so far go out now, beside the chain kernels still to come; from here on a fork per layer
        self.flush_list()
        self.tail = True

    def finish(self):
        """What a sweep shorter than the tail rule left, then the chain's stream waits for every side stream."""
        self.tail = False
        self.flush_list()
        self.ops.mark("student.bwd.main.end")
        for side in self.streams():
            torch.cuda.current_stream().wait_stream(side)
