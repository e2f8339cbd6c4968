"""The split tuner, the in-flight window and the refinement's resets (csrc/rtx_policy.h) as a Python
model — TEST INFRASTRUCTURE (tests/test_policy_cpu.py).  Written from the structs' comments and
DESIGN.md §3 / §6, not from their code; numpy.float32 wherever the C++ computes in float.

The tuner: a timed frame (main kernel and split chain, ms, both from the fork) rendered the heavy set
selected with factor `base` (permille).  The pair is kept.  Non-positive times, base 0 and a base that
is not the current factor are ignored.  The span max(main, chain) becomes the best when it is the first
or smaller than the best; a span more than 5 % above the best returns to the best's factor: done.
Otherwise chain / main within 4 % of 1: done; the 17th step: done; else the step (1.15 at first) becomes
its square root when the direction changed, and a step under 1.015: done; else the factor is base x step
(chain longer) or base / step, in double, clamped to 1000..4000 and truncated.

The window: per call the slot is cleared; threshold 0: split; ratio known (> 0) and ratio x 1000 under
the threshold: one piece.  Neither touches the window.  Then by state: 4 (done) — one piece iff span and
interval are known and k x span < 1.15 x interval; 0 — the 16th such frame starts timing (state 2, slot
0); 2 — the 32nd ends it (state 3, slot 1); 3 — once the end event is ready, interval = elapsed / 32
when elapsed > 0, state 4.  All but state 4: split."""
from __future__ import annotations

import numpy as np

F = np.float32
SPLIT_PERMILLE, WINDOW, WINDOW_SKIP, REFINE_QUIET = 1500, 32, 16, 32
OVERLAP_MIN = F(1.15)


def bits(x) -> str:
    return f"{int(np.asarray(F(x)).view(np.uint32)):08x}"


class Tuner:
    def __init__(self):
        self.permille, self.on, self.done, self.rec = SPLIT_PERMILLE, True, False, False
        self.main, self.chain = F(0), F(0)
        self._search()

    def _search(self):
        self.done, self.steps, self.dir, self.step_size = False, 0, 0, F(1.15)
        self.best, self.best_permille = F(0), 0

    def restart_default(self):
        """A new launch shape: a tuner that is on searches again from the default factor; the timing in
        flight is dropped either way."""
        if self.on:
            self.permille = SPLIT_PERMILLE
            self._search()
        self.rec = False

    def restart_here(self):
        """A shorter chain: a tuner that is on searches again from the factor it has."""
        if self.on:
            self._search()

    def step(self, base: int, main, chain):
        main, chain = F(main), F(chain)
        self.main, self.chain = main, chain
        if base == 0 or main <= 0 or chain <= 0 or base != self.permille:
            return
        span = max(main, chain)
        if self.best_permille == 0 or span < self.best:
            self.best, self.best_permille = span, base
        elif span > F(1.05) * self.best:
            self.permille, self.done = self.best_permille, True
            return
        r = chain / main
        d = 1 if r > F(1.04) else (-1 if r < F(0.96) else 0)
        if d != 0:
            self.steps += 1
        if d == 0 or self.steps > 16:
            self.done = True
            return
        if self.dir != 0 and d != self.dir:
            self.step_size = np.sqrt(self.step_size)
        if self.step_size < F(1.015):
            self.done = True
            return
        self.dir = d
        f = float(base) * (float(self.step_size) if d > 0 else 1.0 / float(self.step_size))
        self.permille = int(min(4000.0, max(1000.0, f)))

    def line(self) -> str:
        return (f"t permille={self.permille} on={int(self.on)} done={int(self.done)} rec={int(self.rec)} "
                f"steps={self.steps} dir={self.dir} step={bits(self.step_size)} main={bits(self.main)} "
                f"chain={bits(self.chain)} best={bits(self.best)} best_permille={self.best_permille}")


class Window:
    def __init__(self):
        self.state, self.frames, self.rec, self.interval = 0, 0, -1, F(0)
        self.wants, self.one = False, False

    def reset(self):
        self.state, self.frames, self.interval = 0, 0, F(0)
        self.wants = self.one = False

    def onepiece(self, crit: int, ratio, k: int, span, ready: bool, elapsed) -> bool:
        ratio, span, elapsed = F(ratio), F(span), F(elapsed)
        short = ratio > 0 and ratio * F(1000) < F(crit)
        self.wants = crit != 0 and not short and self.state == 3   # the end event is asked for only here
        self.one = self._decide(crit, short, k, span, ready, elapsed)
        return self.one

    def _decide(self, crit, short, k, span, ready, elapsed) -> bool:
        self.rec = -1
        if crit == 0:
            return False
        if short:
            return True
        if self.state == 4:
            return bool(span > 0 and self.interval > 0 and F(k) * span < OVERLAP_MIN * self.interval)
        if self.state == 0:
            self.frames += 1
            if self.frames >= WINDOW_SKIP:
                self.state, self.frames, self.rec = 2, 0, 0
        elif self.state == 2:
            self.frames += 1
            if self.frames == WINDOW:
                self.state, self.rec = 3, 1
        elif self.state == 3 and ready:
            if elapsed > 0:
                self.interval = elapsed / F(WINDOW)
            self.state = 4
        return False

    def line(self) -> str:
        return (f"w wants={int(self.wants)} one={int(self.one)} state={self.state} frames={self.frames} "
                f"rec={self.rec} interval={bits(self.interval)}")


class Refine:
    def __init__(self):
        self.round, self.state, self.wait, self.quiet, self.prev_max, self.rec = 0, 2, 0, 0, 0, False

    def reset_shape(self):
        """A new launch shape (of a refinable scene): round 0, waiting, REFINE_QUIET frames of quiet, no
        measurement in flight."""
        self.round, self.state, self.wait, self.prev_max, self.rec, self.quiet = 0, 0, 0, 0, False, REFINE_QUIET

    def reset_upload(self, refinable: bool):
        """An upload: round 0, waiting (done when not refinable); the quiet frames and a measurement in
        flight are left alone."""
        self.round, self.state, self.wait, self.prev_max = 0, (0 if refinable else 2), 0, 0

    def line(self) -> str:
        return (f"r round={self.round} state={self.state} wait={self.wait} quiet={self.quiet} "
                f"prev_max={self.prev_max} rec={int(self.rec)}")


def run(script: list[str]) -> list[str]:
    """The trace of tests/policy_harness.cpp for the same script (its grammar is in that file)."""
    t, w, r, out = Tuner(), Window(), Refine(), []
    for ln in script:
        who, what, *a = ln.split()
        if who == "t":
            if what == "step":
                t.step(int(a[0]), float.fromhex(a[1]), float.fromhex(a[2]))
            elif what == "default":
                t.restart_default()
            elif what == "here":
                t.restart_here()
            elif what in ("on", "rec"):
                setattr(t, what, a[0] != "0")
            elif what == "permille":
                t.permille = int(a[0])
            else:
                raise ValueError(ln)
            out.append(t.line())
        elif who == "w":
            if what == "one":
                w.onepiece(int(a[0]), float.fromhex(a[1]), int(a[2]), float.fromhex(a[3]), a[4] != "0", float.fromhex(a[5]))
            elif what == "reset":
                w.reset()
            else:
                raise ValueError(ln)
            out.append(w.line())
        elif who == "r":
            if what == "shape":
                r.reset_shape()
            elif what == "upload":
                r.reset_upload(a[0] != "0")
            elif what == "set":
                r.round, r.state, r.wait, r.quiet, r.prev_max = (int(x) for x in a[:5])
                r.rec = a[5] != "0"
            else:
                raise ValueError(ln)
            out.append(r.line())
        else:
            raise ValueError(ln)
    return out
