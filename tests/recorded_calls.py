"""What the tests read off a pass recorded with `scoring._CallRecorder`: the sweep is ONE entry per launch sequence
(include/polara_hip.h), so the route a pass took is a statement about the recorded arguments of that call."""

SWEEP_ENTRIES = {'pk_score_candidates_f32': 27, 'pk_score_two_phase_f32': 29}     # entry -> number of arguments


def given(arg):
    """is this recorded pointer argument (a ctypes pointer, or None) non-null?"""
    return arg is not None and bool(getattr(arg, 'value', arg))


def sweeps(calls):
    """the sweep calls among recorded (name, fn, args) triples, each as a dict: the entry, and which of the users' side
    (arguments 5-12: Ep, user_bound | E, lde, extra, extra_ld, extra_scale, user_bound_out) and of the settle block (the
    single sweep's last argument; the two-phase sweep has none) was given"""
    out = []
    for name, _, a in calls:
        if name in SWEEP_ENTRIES:
            assert len(a) == SWEEP_ENTRIES[name], (name, len(a))
            out.append(dict(entry=name, Ep=given(a[5]), user_bound=given(a[6]), E=given(a[7]), extra=given(a[9]),
                            user_bound_out=given(a[12]), settle=name == 'pk_score_candidates_f32' and given(a[26])))
    return out
