"""Fork / join of jobs that run on side HIP streams next to the caller's stream.

The choreography the three models share: an event recorded on ``main`` where the jobs fork, every side stream waits on it
before its job, records its own event after it, and ``main`` waits on those only after EVERY job has been enqueued (joining
earlier would serialise the jobs).  The streams, what runs between ``begin`` and ``end`` and whether it runs under
``torch.cuda.stream(st)`` stay with the caller.
"""
from __future__ import annotations

import torch


class SideJobs:
    def __init__(self, main):
        self.main, self.done = main, []
        self.fork = torch.cuda.Event()
        self.fork.record(main)

    def begin(self, st):
        if st is not self.main:
            st.wait_event(self.fork)

    def end(self, st):
        if st is not self.main:
            ev = torch.cuda.Event()
            ev.record(st)
            self.done.append(ev)

    def join(self):
        for ev in self.done:
            self.main.wait_event(ev)
