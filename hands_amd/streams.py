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


def run_crop_chunks(main, nch, n, side_stream, job):
    """Rows [0, n) cut into ``nch`` (1 <= nch <= n) jobs ``job(lo, hi, st, ci)`` that run side by side: the last (largest) chunk on
    ``main``, chunk ci of the others on ``side_stream(ci)``, each under ``torch.cuda.stream(st)``, forked and joined through
    :class:`SideJobs`.  One chunk runs on ``main`` as it is: no events, no stream switch.  Returns the jobs' results in order."""
    if nch == 1:
        return [job(0, n, main, 0)]
    jobs, parts = SideJobs(main), []
    for ci in range(nch):
        st = main if ci == nch - 1 else side_stream(ci)
        jobs.begin(st)
        with torch.cuda.stream(st):
            parts.append(job(ci * n // nch, (ci + 1) * n // nch, st, ci))
        jobs.end(st)
    jobs.join()
    return parts
