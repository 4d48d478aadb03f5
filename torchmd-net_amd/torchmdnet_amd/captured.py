"""What every captured HIP graph of this package shares: the capture sequence, the stale-graph guard and the base of the loop objects.

A captured graph records raw device pointers: of every input, of the engine's parameter block and of its workspaces.  Two rules follow,
and each is written once, here or in ``TorchMD_Net._capture_inputs``:

1. the inputs are brought to the device and dtype the engine takes BEFORE the capture and are kept alive by whoever holds the graph
   (``inputs``); a conversion inside the captured call would be a temporary, and the replay would read freed memory
   (``TorchMD_Net._capture_inputs``);
2. the engine's own memory is re-created by an eager call after a parameter change or a device move, or with a larger system; a replay
   after that must raise, not touch freed memory (``engine_token`` / ``check_fresh``).

A third lifetime of the same family is not handled here yet: atom weights passed to a captured evaluation are kept alive by the
engine itself, ``engine.captured_atom_weights`` (``TorchMD_Net.energy_and_forces``), a list bounded to the last 8 captures, so a
ninth capture evicts the vector of the first while its graph can still be replayed.  The list belongs with ``inputs`` of whoever
holds the graph; the loops below refuse atom weights, so only ``capture`` through ``energy_and_forces`` is affected."""
import ctypes as C

import torch

from torchmdnet_amd import _C
from torchmdnet_amd.models.utils import _ptr, _stream_ptr


def capture_graph(dev, warm, record, warmup=3, start=None, before_capture=None):
    """The capture sequence on ``dev``: on a side stream ``max(warmup, 1)`` calls of ``warm()`` (they upload the parameters, size the
    workspaces and check overflow) and then ``start(out)`` with the last call's result (what a loop enqueues once before its first
    step); join back to the current stream; ``before_capture()`` there (a read-back that must not be recorded); then ``record()``
    inside ``torch.cuda.graph``.  -> the graph"""
    with torch.cuda.device(dev):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):
                out = warm()
            if start is not None:
                start(out)
        torch.cuda.current_stream(dev).wait_stream(side)
        if before_capture is not None:
            before_capture()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            record()
    return graph


def engine_token(model):
    """What a graph captured from ``model`` points into: the engine object and its generation, as they are now"""
    st = model._engine
    return st, st.generation


def check_fresh(now, captured, what, again="capture again"):
    """Raise when the token taken at the capture is no longer the current one: replaying would touch freed memory"""
    if now != captured:
        raise RuntimeError(f"stale HIP graph: the model's parameters or workspaces changed after {what}; {again}")


class CapturedLoop:
    """Base of the loop objects (``DeviceMD``, ``DeviceMinimizer``, ``DeviceNEB``): K steps in one graph, replayed by ``loop(n)``.
    A subclass sets ``_capture_name`` and ``_noun``, stages its state (``pos``, ``_ws``, ``inputs``), provides ``_evaluate()`` and
    ``_capture_step(k, K, out)`` and calls ``_capture`` last in its constructor."""

    _capture_name = "capture"  # the method of TorchMD_Net that makes the object, for the messages
    _noun = "the state"        # what the overflow error says is frozen

    def __init__(self, model, steps_per_replay):
        self._model = model
        self.steps_per_replay = int(steps_per_replay)
        self.steps_done = 0
        self.graph, self._step_outputs, self._token = None, [], None

    def _capture(self, warmup, start, open_step, before_capture=None):
        """``capture_graph``: ``_evaluate`` warms up, ``start(out)`` follows it, and the graph records ``open_step()`` and then, K
        times, an evaluation and ``_capture_step(k, K, out)``.  The evaluations' output buffers live in the graph's pool; they are
        kept for the graph's lifetime."""
        K = self.steps_per_replay

        def record():
            open_step()
            for k in range(K):
                out = self._evaluate()
                self._step_outputs.append(out)
                self._capture_step(k, K, out)

        self.graph = capture_graph(self.pos.device, self._evaluate, record, warmup, start, before_capture)
        self._token = engine_token(self._model)

    def _check_fresh(self):
        check_fresh(engine_token(self._model), self._token, f"{self._capture_name}()")

    def __call__(self, n: int = 1):
        self._check_fresh()
        for _ in range(int(n)):
            self.graph.replay()
        self.steps_done += int(n) * self.steps_per_replay
        return self

    def _status(self, entry, words):
        """One of the C status entries on this loop's workspace (one synchronisation) -> (rc, [words] ints); word 0 is the device's
        step counter"""
        host = (C.c_uint64 * words)()
        dev = self.pos.device
        with torch.cuda.device(dev):
            rc = entry(_stream_ptr(dev), _ptr(self._ws), C.cast(host, C.POINTER(C.c_uint64)))
        return rc, [int(w) for w in host]

    def _overflow(self, step):
        """The reference's overflow error, for a status entry that answered ERR_OVERFLOW"""
        return RuntimeError("Found num_pairs > max_num_pairs, please increase max_num_pairs "
                            f"(max_num_neighbors={self._model.representation_model.max_num_neighbors}; {self._noun} is frozen at "
                            f"step {step})")

    def _verdict(self, entry, rc, step, status, cause=0, label=None, causes=None):
        """What ``check()`` makes of the answer of the status entry named ``entry``: the step counter, or the reference's overflow
        error, or - status 2 of a loop that gives its ``label`` - the error naming the cause (``causes``: cause -> text), or the
        entry's failure.  A loop whose messages have another shape raises them itself and passes no label."""
        if rc == _C.ERR_OVERFLOW:
            raise self._overflow(step)
        if status == 2 and label is not None:
            why = (causes or {}).get(cause, "a sum is not finite")
            raise RuntimeError(f"{label}: after step {step} {why}; the state is frozen at that step")
        if rc != _C.OK:
            raise RuntimeError(f"{entry} failed (code {rc})")
        return step

    def _reset(self, copy_in, start, step=0):
        """The skeleton of every ``reset``: ``copy_in()`` validates and then writes the static buffers, the evaluation there raises
        when these positions overflow, ``start(out)`` enqueues what the capture enqueued after its warm-up, and the evaluation must
        not have re-created what the graph points into."""
        self._check_fresh()
        copy_in()
        out = self._evaluate()
        with torch.cuda.device(self.pos.device):
            start(out)
        self.steps_done = int(step)
        self._check_fresh()
        return self


class ConvergingLoop(CapturedLoop):
    """A loop whose units (molecules, bands) stop at their own step: ``converged_at`` [units] int64, -1 while a unit still moves"""

    def run(self, max_steps: int, check_every: int = 1) -> int:
        """Replay until every molecule (band) has converged or another replay would exceed ``max_steps`` steps; ``converged_at`` is
        read back (one synchronisation) before the first replay and then after every ``check_every`` replays.  Steps come in whole
        replays of ``steps_per_replay``.  Returns the number of steps taken by this call; ``check()`` tells whether they were valid."""
        K, every = self.steps_per_replay, max(int(check_every), 1)
        taken = 0
        while not bool((self.converged_at >= 0).all()):
            n = min(every, (int(max_steps) - taken) // K)
            if n < 1:
                break
            self(n)
            taken += n * K
        return taken
