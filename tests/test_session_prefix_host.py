"""Page prefix cache, host side (no GPU): the C ABI exports, the scheduler's key / LRU / bypass rules against a
scripted engine, and the server flag."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from dsocr import DecodeParameters, VisionSettings
from dsocr import server
from dsocr.synth import SyntheticTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dsocr_session_prefix_keep", "dsocr_session_admit_prefix", "dsocr_session_prefix_drop",
               "dsocr_session_prefix_stats", "dsocr_k_prefill_attention_past", "dsocr_k_session_prefix_copy"]


def test_c_abi_exports_the_prefix_symbols():
    header = open(os.path.join(ROOT, "include", "dsocr.h")).read()
    declared = set(re.findall(r"\b(dsocr_[a-z0-9_]+)\s*\(", header))
    from dsocr._lib import EXPORTS, LIB_PATH
    L = C.CDLL(LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in EXPORTS, s
        assert hasattr(L, s), s


def test_python_session_has_the_prefix_methods():
    from dsocr.engine import Session
    for m in ("keep_prefix", "admit_prefix", "drop_prefix", "prefix_stats"):
        assert callable(getattr(Session, m)), m


# ------------------------------------------------------------------ a scripted engine
class Status:
    def __init__(self, slot, done, out_len, new_tokens):
        self.slot, self.done, self.out_len, self.new_tokens = slot, done, out_len, new_tokens


class FakeSession:
    """Every admission yields `n_tokens` tokens of its key, one at the admission and one per step.  The log records
    admissions (plain / prefix), keeps and drops."""
    burst_cap = 8

    def __init__(self, eng, slots, max_context, params):
        self.eng, self.slots, self.out_cap = eng, slots, params.max_new_tokens
        self.kv_cap = max_context + self.burst_cap
        self.active, self.handles, self.next_handle = [], {}, 1

    def _slot(self, ids, kind):
        key = ids[-1]
        self.active.append(dict(key=key, pos=1, reported=0))
        self.eng.log.append((kind, key, len(self.active) - 1))
        return len(self.active) - 1

    def admit(self, ids, mask=None, page=None, image_rows=None, max_new_tokens=None, seed=None):
        return self._slot(ids, "admit")

    def admit_prefix(self, handle, ids, mask=None, max_new_tokens=None, seed=None):
        if self.eng.refuse_prefix:
            raise RuntimeError("scripted refusal")
        rows, pre = self.handles[handle]  # KeyError: a dropped or unknown handle
        assert list(ids[:rows]) == pre and len(ids) > rows and not any(mask[rows:])
        self.eng.log.append(("use", handle))
        return self._slot(ids, "admit_prefix")

    def keep_prefix(self, slot, rows):
        assert 0 <= slot < len(self.active) and rows >= 1
        if self.eng.refuse_keep:
            raise MemoryError("scripted ENOMEM")
        h = self.next_handle
        self.next_handle += 1
        self.handles[h] = (rows, list(self.eng.last_ids[self.active[slot]["key"]][:rows]))
        self.eng.log.append(("keep", h, slot, rows))
        return h

    def drop_prefix(self, handle):
        del self.handles[handle]
        self.eng.log.append(("drop", handle))

    def poll(self):
        out = []
        for i, s in enumerate(self.active):
            pos = min(s["pos"], self.eng.n_tokens)
            fresh = [1000 * s["key"] + t for t in range(s["reported"], pos)]
            s["reported"] = pos
            out.append(Status(i, s["pos"] >= self.eng.n_tokens, pos, fresh))
        return out

    def step(self, k):
        for s in self.active:
            s["pos"] += k
        return self.poll()

    def retire(self, slot):
        s = self.active[slot]
        last, moved = len(self.active) - 1, -1
        if slot != last:
            self.active[slot] = self.active[last]
            moved = last
        self.active.pop()
        return [1000 * s["key"] + t for t in range(self.eng.n_tokens)], moved

    def close(self):
        self.eng.log.append(("close",))


class FakeEngine:
    variant = 0
    n_tokens = 3
    refuse_prefix = refuse_keep = False

    def __init__(self):
        self.log, self.last_ids = [], {}

    def open_session(self, slots, max_context, params, **kw):
        return FakeSession(self, slots, max_context, params)

    def image_embeddings(self, pages):
        return [np.zeros((4, 8), np.float32) for _ in pages]


def _prepare_for(eng):
    def prepare(engine, tokenizer, prompt, images, vision):
        """prompt "KEY" or "KEY:notext": [BOS] + 4 image rows per image + [7, KEY] (or nothing after the image)"""
        key = int(prompt.split(":")[0])
        ids, mask = [0], [0]
        for _ in images:
            ids += [9] * 4
            mask += [1] * 4
        if not prompt.endswith(":notext"):
            ids += [7, key]
            mask += [0, 0]
        eng.last_ids[ids[-1]] = list(ids)
        return ids, mask, [object() for _ in images]
    return prepare


def _sched(eng, n, **kw):
    from dsocr.scheduler import BatchScheduler
    return BatchScheduler(eng, SyntheticTokenizer(512), 2, 128, DecodeParameters(max_new_tokens=8),
                          VisionSettings(256, 128, True), prepare=_prepare_for(eng), prefix_cache=n, **kw)


def _img(seed):
    return np.random.default_rng(seed).integers(0, 256, (8, 8, 3), dtype=np.uint8)


def _run(s, prompt, images, **kw):
    return s.submit(prompt, images, **kw).result(timeout=20)


def test_same_image_hits_and_other_images_or_settings_miss():
    eng = FakeEngine()
    a, b = _img(1), _img(2)
    with _sched(eng, 4) as s:
        _run(s, "11", [a])
        _run(s, "12", [a.copy()])                                          # the same pixels: a hit
        _run(s, "13", [b])                                                 # another image: a miss
        _run(s, "14", [a], vision=VisionSettings(256, 128, False))         # other vision settings: a miss
        _run(s, "15", [a], vision=VisionSettings(256, 128, False))         # ... and a hit under those
        assert (s.prefix_hits, s.prefix_misses) == (2, 3)
    kinds = [(e[0], e[1]) for e in eng.log if e[0] in ("admit", "admit_prefix")]
    assert kinds == [("admit", 11), ("admit_prefix", 12), ("admit", 13), ("admit", 14), ("admit_prefix", 15)]
    keeps = [e for e in eng.log if e[0] == "keep"]
    assert len(keeps) == 3 and all(e[3] == 5 for e in keeps)               # rows: BOS + the four image rows
    uses = [e[1] for e in eng.log if e[0] == "use"]
    assert uses == [keeps[0][1], keeps[2][1]]


def test_lru_eviction_drops_the_handle_before_the_next_keep():
    eng = FakeEngine()
    a, b, c = _img(1), _img(2), _img(3)
    with _sched(eng, 2) as s:
        _run(s, "21", [a])
        _run(s, "22", [b])
        _run(s, "23", [a])      # a hit: `a` is now the most recently used
        _run(s, "24", [c])      # evicts b
        _run(s, "25", [b])      # a miss again; evicts a
        _run(s, "26", [c])      # still cached
        assert (s.prefix_hits, s.prefix_misses) == (2, 4)
    keeps = {e[1]: i for i, e in enumerate(eng.log) if e[0] == "keep"}
    drops = [(i, e[1]) for i, e in enumerate(eng.log) if e[0] == "drop"]
    assert [h for _, h in drops] == [2, 1]                                  # b's handle, then a's
    assert drops[0][0] < keeps[3] and drops[1][0] < keeps[4]                # dropped before the keep that needed room
    # (a dropped handle is never used again: FakeSession.admit_prefix would raise through the request's future)


def test_bypass_rules_and_the_default():
    eng = FakeEngine()
    a, b = _img(1), _img(2)
    with _sched(eng, 4) as s:
        _run(s, "31", [a, b])            # several images: never cached
        _run(s, "32", [a, b])
        _run(s, "33:notext", [a])        # nothing after the image: no new row to take the logits from
        _run(s, "33:notext", [a])
        _run(s, "34", [])                # no image
        assert (s.prefix_hits, s.prefix_misses) == (0, 0)
    assert not any(e[0] in ("keep", "admit_prefix") for e in eng.log)
    eng = FakeEngine()
    with _sched(eng, 0) as s:            # the default: the cache is off
        _run(s, "41", [a])
        _run(s, "42", [a])
        assert (s.prefix_hits, s.prefix_misses) == (0, 0) and s.prefix_cache == 0
    assert [e[0] for e in eng.log if e[0] != "close"] == ["admit", "admit"]
    from dsocr.scheduler import BatchScheduler
    import inspect
    assert inspect.signature(BatchScheduler.__init__).parameters["prefix_cache"].default == 0
    with pytest.raises(ValueError):
        _sched(FakeEngine(), 65)


def test_exclusive_requests_bypass_the_cache():
    eng = FakeEngine()
    eng.decode = lambda tokenizer, prompt, images, vision, params, stream=None: __import__("dsocr").DecodeOutcome(
        "", 7, 1, [5])
    a = _img(1)
    with _sched(eng, 4) as s:
        _run(s, "51", [a])
        out = _run(s, "52", [a], params=DecodeParameters(max_new_tokens=8, repetition_penalty=1.3))
        assert out.generated_tokens == [5] and s.exclusive_runs == 1
        assert (s.prefix_hits, s.prefix_misses) == (0, 1)


def test_refused_prefix_admission_falls_back_and_failed_keeps_are_counted():
    eng = FakeEngine()
    a, b = _img(1), _img(2)
    with _sched(eng, 4) as s:
        _run(s, "61", [a])
        eng.refuse_prefix = True
        out = _run(s, "62", [a])                 # a hit whose admit_prefix is refused: admitted plainly instead
        assert out.response_tokens == eng.n_tokens
        assert (s.prefix_hits, s.prefix_fallbacks, s.prefix_misses) == (1, 1, 1)
        eng.refuse_keep = True
        _run(s, "63", [b])                       # the keep fails: the request is served, the failure is counted
        assert (s.prefix_misses, s.prefix_keep_failures) == (2, 1)
    assert [(e[0], e[1]) for e in eng.log if e[0].startswith("admit")] == [("admit", 61), ("admit", 62), ("admit", 63)]


def test_server_flag(capsys):
    import argparse
    p = argparse.ArgumentParser()
    server.add_scheduler_args(p)
    assert p.parse_args([]).prefix_cache == 0
    assert p.parse_args(["--slots", "4", "--prefix-cache", "16"]).prefix_cache == 16
    st = server.ServerState(FakeEngine(), SyntheticTokenizer(512), "deepseek-ocr", VisionSettings(256, 128, True),
                            DecodeParameters(max_new_tokens=8))
    with pytest.raises(ValueError, match="--slots"):
        server.make_scheduler(st, 0, 128, prefix_cache=4)
    on = server.make_scheduler(st, 2, 128, prefix_cache=4)
    try:
        assert on.prefix_cache == 4
    finally:
        on.close()
    with pytest.raises(ValueError, match="0..64"):
        server.make_scheduler(st, 2, 128, prefix_cache=65)
    # the command line refuses both before anything is loaded, and for this reason
    for argv in (["--prefix-cache", "4"], ["--slots", "2", "--prefix-cache", "65"]):
        with pytest.raises(SystemExit):
            server.main(argv)
        assert "--prefix-cache needs --slots and N in 0..64" in capsys.readouterr().err
