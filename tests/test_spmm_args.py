"""The argument rules of the three row-task product entries, pk_spmm_csr_ex, pk_spmm_csr_flagged_f64 and
pk_spmm_csr_rows_list_f64 (include/polara_hip.h): each rule is rejected before anything is launched, with a message that starts
with the entry's name.  No device is needed — the entries check before they touch the stream, and the stand-in pointers below
are never dereferenced on the host.

EVERY call in this file is a rejected one.  The calls of the plain and the flagged entry carry n_tasks = 0: both return PK_OK
for an empty task list after their checks and before any launch, so a case that slipped through the rule it aims at would fail
its assertion, not start a kernel over made-up addresses.  The listed entry has no such exit: its calls carry a bad val_kind
besides the rule they are about — the value kind is the LAST check of the shared validator, so the message is still the
aimed-at rule's, and a case that slipped through it ends at the value kind.  (That rule itself is the shared validator's and
is shown through the other two entries.)"""
import pytest

P = [0x1000 * (i + 1) for i in range(16)]        # distinct, 16-byte aligned, never dereferenced
PLAIN, FLAGGED, LISTED = 'pk_spmm_csr_ex', 'pk_spmm_csr_flagged_f64', 'pk_spmm_csr_rows_list_f64'
E_INVALID, E_UNSUPPORTED = -1, -3                 # include/polara_hip.h
PLAN = ('task_row', 'task_begin', 'task_end', 'task_slot', 'n_long', 'long_row', 'long_slot_begin', 'long_slot_end')
ORDER = {
    PLAIN: ('stream', 'n_tasks') + PLAN + ('indices', 'vals', 'val_kind', 'X', 'x_kind', 'ldx', 'nc', 'out', 'ldo', 'partial',
                                           'row_base', 'accumulate', 'x_rows'),
    FLAGGED: ('stream', 'n_tasks') + PLAN + ('indices', 'vals', 'val_kind', 'X', 'ldx', 'nc', 'out', 'ldo', 'partial', 'x_rows',
                                             'row_flags', 'flag_mask'),
    LISTED: ('stream', 'cap', 'list', 'count', 'row_offset', 'row_first_task') + PLAN + (
        'indices', 'vals', 'val_kind', 'X', 'ldx', 'nc', 'out', 'ldo', 'partial', 'x_rows', 'row_flags', 'flag_mask'),
}
N_ARGS = {PLAIN: 23, FLAGGED: 22, LISTED: 26}
BASE = dict(stream=None, n_tasks=0, task_row=P[0], task_begin=P[1], task_end=P[2], task_slot=P[3], n_long=0, long_row=P[4],
            long_slot_begin=P[5], long_slot_end=P[6], indices=P[7], vals=P[8], val_kind=0, X=P[9], x_kind=1, ldx=64, nc=64,
            out=P[10], ldo=64, partial=P[11], row_base=0, accumulate=0, x_rows=1000, row_flags=P[12], flag_mask=7,
            cap=100, list=P[13], count=P[14], row_offset=0, row_first_task=P[15])
BAD_VAL_KIND = 2


def rejected(entry, says, code=E_INVALID, **change):
    from polara_amd import _lib
    lib = _lib.load()
    a = dict(BASE, **change)
    if entry == LISTED:
        a['val_kind'] = BAD_VAL_KIND
    else:
        assert a['n_tasks'] == 0
    args = [a[name] for name in ORDER[entry]]
    assert len(args) == len(_lib.PROTOTYPES[entry][1]) == N_ARGS[entry]
    rc = getattr(lib, entry)(*args)
    msg = (lib.pk_last_error() or b'').decode()
    assert rc != 0 and rc == code, (entry, change, rc)
    assert msg.startswith(entry + ': ') and says in msg, (entry, change, msg)


# rules of the shared validator: (what the message says, the change that breaks the rule)
SHARED = [
    ('bad sizes', dict(nc=0)),
    ('bad sizes', dict(nc=258, ldx=258, ldo=258)),
    ('ldo/ldx < nc', dict(ldo=62)),
    ('ldo/ldx < nc', dict(ldx=62)),
    ('partial buffer required', dict(n_long=1, partial=None)),
]
# the two entries that take an fp64 block only: even nc and ldx, X 16-byte aligned
F64_ONLY = [
    ('even, 2..256', dict(nc=7)),
    ('even, 2..256', dict(nc=63)),
    ('ldx even, X 16-byte aligned', dict(ldx=65)),
    ('ldx even, X 16-byte aligned', dict(X=P[9] + 8)),
]


@pytest.mark.parametrize('entry', [PLAIN, FLAGGED, LISTED])
def test_shared_argument_rules_are_rejected_before_any_launch(entry):
    for says, change in SHARED + (F64_ONLY if entry != PLAIN else []):
        rejected(entry, says, **change)


@pytest.mark.parametrize('entry', [PLAIN, FLAGGED])
def test_value_kind_is_checked_for_an_empty_task_list_too(entry):
    rejected(entry, 'bad val_kind 2', val_kind=BAD_VAL_KIND)
    rejected(entry, 'bad val_kind -1', val_kind=-1)


def test_plain_product_rules():
    rejected(PLAIN, 'bad sizes', nc=257, ldx=260, ldo=260)           # (odd widths are the plain entry's alone: 257 is too wide)
    rejected(PLAIN, 'bad x_kind 2', x_kind=2)
    rejected(PLAIN, 'a row base needs accumulate', row_base=5)
    rejected(PLAIN, 'a row base needs accumulate', row_base=-1, accumulate=1)
    # the fp32 dense block: one 16-byte load = 4 columns; its own error code
    for change in (dict(nc=6), dict(nc=62), dict(ldx=66), dict(X=P[9] + 4), dict(X=P[9] + 8)):
        rejected(PLAIN, 'fp32 dense block', code=E_UNSUPPORTED, x_kind=0, **change)
    # it has the row base, the accumulate switch and the kind of X besides the flagged entry's arguments, not the flags
    assert len(ORDER[PLAIN]) == len(ORDER[FLAGGED]) + 3 - 2


def test_flagged_product_rules():
    rejected(FLAGGED, 'row flags required', row_flags=None)


def test_listed_product_rules():
    rejected(LISTED, 'bad val_kind 2')                                 # (nothing else broken: what every other case here ends at)
    rejected(LISTED, 'bad sizes', cap=0)
    for ptr in ('list', 'count', 'row_first_task', 'task_row'):
        rejected(LISTED, 'bad pointers', **{ptr: None})
    rejected(LISTED, 'split rows need the row flags', n_long=1, row_flags=None)
