"""The per-coding-thread state and job threads of the frame path (pcc_amd._threads; no GPU needed)."""
import threading
import time

import numpy as np
import pytest


def _gone(threads, timeout=5.0):
    """wait until none of ``threads`` is among the live threads"""
    deadline = time.monotonic() + timeout
    while set(threads) & set(threading.enumerate()):
        if time.monotonic() > deadline:
            return False
        time.sleep(0.01)
    return True


def test_jobs_run_in_submission_order(pcc):
    from pcc_amd import _threads
    jt = _threads.JobThread("pcc-test-order")
    seen = []
    dones = [jt.submit(lambda i=i: seen.append(i) or i) for i in range(50)]
    assert [d.wait() for d in dones] == list(range(50))
    assert seen == list(range(50))
    jt.close()
    jt.thread.join(5)
    assert not jt.thread.is_alive()


def test_an_error_in_a_job_is_reraised_by_wait_and_the_thread_goes_on(pcc):
    from pcc_amd import _threads
    jt = _threads.JobThread("pcc-test-error")

    def failing():
        raise KeyError("raised in the job")

    bad = jt.submit(failing)
    with pytest.raises(KeyError, match="raised in the job"):
        bad.wait()
    with pytest.raises(KeyError):                    # every wait re-raises it
        bad.wait()
    assert jt.submit(lambda: threading.current_thread() is jt.thread).wait()
    jt.close()


def test_threads_get_distinct_states_and_one_thread_the_same(pcc):
    from pcc_amd import _threads
    here = _threads.current()
    assert _threads.current() is here
    there = []
    t = threading.Thread(target=lambda: there.extend([_threads.current(), _threads.current()]))
    t.start()
    t.join()
    assert there[0] is there[1] and there[0] is not here


def test_an_ended_thread_leaves_no_job_thread_behind(pcc):
    from pcc_amd import entropy
    before = {t for t in threading.enumerate() if t.name == "pcc-rans"}          # (the main thread may own one)
    made = []

    def coding_thread():
        jt = entropy._rans_thread()
        assert jt is entropy._rans_thread()
        made.append(jt.thread)
        assert jt.submit(lambda: 7).wait() == 7

    for _ in range(4):
        t = threading.Thread(target=coding_thread)
        t.start()
        t.join()
    assert len(made) == 4 and all(t.name == "pcc-rans" for t in made) and not set(made) & before
    assert _gone(made)


def test_a_job_thread_starts_no_job_threads(pcc):
    from pcc_amd import _threads
    jt = _threads.JobThread("pcc-test-nested")
    st = jt.submit(_threads.current).wait()
    assert st is not _threads.current()
    with pytest.raises(RuntimeError, match="does not start job threads"):
        jt.submit(lambda: _threads.current().job_thread("pcc-rans")).wait()
    jt.close()


def test_channel_index_plane_evicts_one_entry_at_a_time(pcc):
    from pcc_amd import entropy
    plane = entropy._channel_index_plane
    plane.cache_clear()
    first = plane(3, 5)
    assert first.dtype == np.int32 and np.array_equal(first, np.repeat(np.arange(3, dtype=np.int32), 5))
    for n in range(6, 6 + 63):
        plane(3, n)
    assert plane.cache_info().currsize == 64 and plane(3, 5) is first
    plane(3, 100)                                     # one past the size: the least recently used entry (3, 6) goes, no more
    assert plane.cache_info().currsize == 64
    misses = plane.cache_info().misses
    assert plane(3, 5) is first
    plane(3, 7)
    assert plane.cache_info().misses == misses
    plane(3, 6)
    assert plane.cache_info().misses == misses + 1


def test_an_array_a_job_holds_survives_eviction(pcc):
    import weakref
    from pcc_amd import _threads, entropy
    plane = entropy._channel_index_plane
    plane.cache_clear()
    jt = _threads.JobThread("pcc-test-hold")
    gate = threading.Event()
    held = plane(4, 1000)
    alive = weakref.ref(held)

    def work(_held=(held,)):                         # the decode jobs' shape: the arrays ride on the job
        gate.wait()
        return int(_held[0].sum())

    done = jt.submit(work)
    del work, held
    for n in range(2000, 2000 + 80):                 # evicts (4, 1000) from the cache
        plane(4, n)
    assert plane.cache_info().currsize == 64 and alive() is not None
    gate.set()
    assert done.wait() == 1000 * (0 + 1 + 2 + 3)
    jt.close()
    plane.cache_clear()
