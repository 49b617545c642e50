"""A child process for switches the library reads once per process (AF_SERIAL_STREAMS, AF_ROLES): `python
tests/switch_child.py CASE OUT.npz` runs one case with the switch in its environment and writes the case's arrays.  The
cases are plain functions: the test runs the same one itself, without the switch, as the reference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "audio-forge_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def full_chain_one_call():
    """64 streams, one call of 40 frames (three suppressor windows): front end + suppressor + EQ + compressor + limiter;
    the engine is closed before the case returns."""
    import signals as S
    from mic_eq_mi import mic_eq_core as core

    audio = S.batch_signal(64, 40)
    eng = core.Engine(48_000.0, 64)
    core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, S.limiter_settings(2.0))
    eng.set_prefilter_enabled(1, 1)
    eng.set_suppressor_enabled(1)
    y = eng.process(audio)
    rows = eng.block_stats().copy()
    eng.close()
    return dict(y=y, rows=rows)


def roles_three_calls():
    """The first case of tests/test_gpu_roles.py on kernel 5."""
    import test_gpu_roles as R

    y, rows, used = R._run([R.ROLES], *R.three_calls())
    return dict(y=y, rows=rows, used=np.asarray(used, dtype=np.int32))


if __name__ == "__main__":
    np.savez(sys.argv[2], **{"full_chain_one_call": full_chain_one_call, "roles_three_calls": roles_three_calls}[sys.argv[1]]())
