"""The host threads of the frame path and what one coding thread owns.

A coding thread (the caller's thread; a streamed sequence runs several on one model) overlaps its host work with the GPU's
through job threads of its own: one per device makes the map-prefetch calls (blocks.py), one runs the serial range coder
(entropy.py).  Those, its side streams, its pinned staging buffers and its row-count word live in one state object per
coding thread (``current()``), kept in thread-local storage: when the coding thread ends the state goes with it and its job
threads are told to stop.
"""
import atexit
import queue
import threading
import weakref

import torch


class Handoff:
    """A result or an exception, set once by one thread and taken by another: ``wait()`` returns the result or re-raises the
    exception on the waiting thread.  Later ``set`` / ``fail`` calls are ignored."""

    def __init__(self):
        self._ready = threading.Event()
        self._result = self._err = None

    def set(self, result=None):
        if not self._ready.is_set():
            self._result = result
            self._ready.set()

    def fail(self, err):
        if not self._ready.is_set():
            self._err = err
            self._ready.set()

    def wait(self):
        self._ready.wait()
        if self._err is not None:
            raise self._err
        return self._result


class JobThread:
    """One daemon thread that runs submitted functions in order, under torch.no_grad() (grad mode is per thread).  With a
    ``device`` it makes that device current first (a new thread starts on device 0); without one it touches no CUDA."""

    def __init__(self, name, device=None):
        self._jobs = queue.SimpleQueue()
        self.thread = threading.Thread(target=_serve, args=(self._jobs, device), name=name, daemon=True)
        self.thread.start()

    def submit(self, fn):
        done = Handoff()
        self._jobs.put((fn, done))
        return done

    def close(self):
        """the thread ends after the jobs already submitted; nothing waits for it here (see _join_closed)"""
        _closed.add(self.thread)
        self._jobs.put(None)


# Threads of closed JobThreads, joined at exit (atexit runs before the interpreter starts finalising): a job thread must not end
# while the process does — its exit then races the teardown of the interpreter and the HIP runtime, and a streamed run that
# ended its coding threads just before exiting aborted at exit.  (An ended thread drops out of the set by itself.)
_closed = weakref.WeakSet()


@atexit.register
def _join_closed():
    for t in list(_closed):
        t.join(timeout=10)


def _serve(jobs, device):
    # (a function of the queue alone: the thread holds neither its JobThread nor the state that owns it)
    _local.serves_jobs = True
    if device is not None:
        torch.cuda.set_device(device)
    with torch.no_grad():
        while True:
            job = jobs.get()
            if job is None:
                return
            fn, done = job
            try:
                done.set(fn())
            except BaseException as e:              # re-raised on the submitting thread by done.wait()
                done.fail(e)


class _State:
    """What one thread owns; every field is built on first use by the module that uses it."""

    def __init__(self, serves_jobs):
        self._serves_jobs = serves_jobs
        self._job_threads = {}
        self.side_streams = {}      # (device, main stream handle) -> torch.cuda.Stream (blocks.py)
        self.pinned = {}            # name -> page-locked staging buffer (entropy.py)
        self.pin_busy = {}          # name -> event behind the last asynchronous upload from that buffer
        self.count = None           # (page-locked int64 tensor, numpy view of it): the row-count word (sparse.py)
        self.lane_buffers = {}      # (name, device) -> device scratch / stream buffer of the lane-parallel y coder (entropy.py)
        self.lane_status = []       # device status words of the lane-parallel y decodes not yet checked (entropy.py)
        # when the owning thread ends; not at exit, where the job threads of the threads still alive stay parked
        weakref.finalize(self, _close_all, self._job_threads).atexit = False

    def job_thread(self, name, device=None):
        jt = self._job_threads.get((name, device))
        if jt is None:
            if self._serves_jobs:
                raise RuntimeError(f"a job thread does not start job threads of its own ({name})")
            jt = self._job_threads[(name, device)] = JobThread(name, device)
        return jt


def _close_all(job_threads):
    for jt in job_threads.values():
        jt.close()


_local = threading.local()


def current():
    """the calling thread's state (created on first use; it touches no CUDA)"""
    st = getattr(_local, "state", None)
    if st is None:
        st = _local.state = _State(getattr(_local, "serves_jobs", False))
    return st
