"""Arrival order for the scheduler's GPU tests."""
from contextlib import contextmanager


@contextmanager
def arriving_together(sched):
    """Every request submitted inside the block is queued before the worker serves the first of them.

    ``submit`` does a request's host work on the caller's thread while the worker admits and decodes whatever is
    already queued, and a tiny page decodes in about the time the next ``submit`` takes: which requests then share the
    session is the host's speed, not the scheduler's doing.  The worker takes the scheduler's condition for every look
    at the queue, so holding it (it is re-entrant: ``submit`` takes it too) makes the block one arrival."""
    with sched._cv:
        yield
