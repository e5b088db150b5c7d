"""The argument rules of the two sweep entries, pk_score_candidates_f32 and pk_score_two_phase_f32 (include/polara_hip.h):
each rule is rejected before anything is launched, with a message that starts with the entry's name.  No device is needed —
the entries check before they touch the stream, and the stand-in pointers below are never dereferenced on the host.

EVERY call in this file is a rejected one.  Besides the rule it is about, a call carries KC = 48 wherever the rule does not
need another list size: the launcher refuses that capacity (16, 32, 64) after all argument checks and before its first
launch, so a case that slipped through the rule it aims at would still end in an error return, not in a kernel over
made-up addresses."""
import ctypes

import pytest

P = [0x1000 * (i + 1) for i in range(24)]        # distinct, 16-byte aligned, never dereferenced
SINGLE, TWO = 'pk_score_candidates_f32', 'pk_score_two_phase_f32'
ORDER = {
    SINGLE: ('stream', 'n_users', 'n_items', 'K', 'Vp', 'Ep', 'user_bound', 'E', 'lde', 'extra', 'extra_ld', 'extra_scale',
             'user_bound_out', 'seen_ptr', 'seen_tiles', 'seen_ntiles', 'KC', 'splits', 'cand_score', 'cand_idx', 'state',
             'tiles_per_chunk', 'tile_bound', 'seen_dense', 'seen_skip', 'dense_tiles', 'settle'),
    TWO: ('stream', 'n_users', 'n_items', 'K', 'Vp', 'Ep', 'user_bound', 'E', 'lde', 'extra', 'extra_ld', 'extra_scale',
          'user_bound_out', 'seen_ptr', 'seen_tiles', 'seen_ntiles', 'KC', 'head_tiles', 'splits', 'work_score', 'work_idx',
          'cand_score', 'cand_idx', 'state', 'tiles_per_chunk', 'tile_bound', 'seen_dense', 'seen_skip', 'dense_tiles'),
}
COMMON = dict(stream=None, n_users=70, n_items=1289, K=50, Vp=P[0], seen_ptr=P[1], seen_tiles=P[2], seen_ntiles=P[3], KC=48,
              splits=1, head_tiles=8, work_score=P[4], work_idx=P[5], cand_score=P[6], cand_idx=P[7], state=P[8],
              tiles_per_chunk=0, tile_bound=P[9], seen_dense=None, seen_skip=None, dense_tiles=0, settle=None)
PACKED = dict(COMMON, Ep=P[10], user_bound=P[11], E=None, lde=0, extra=None, extra_ld=0, extra_scale=0.0, user_bound_out=None)
ROWS = dict(COMMON, Ep=None, user_bound=None, E=P[12], lde=52, extra=P[13], extra_ld=52, extra_scale=1.2e-7, user_bound_out=P[14])


def settle_block(**kw):
    from polara_amd import _lib
    f = dict(topk=10, vmax=1.0, item_norm=P[15], out_idx=P[16], out_perm=None, flags=P[17], open_list=P[18], open_count=P[19])
    f.update(kw)
    return _lib.PkSweepSettle(f['topk'], f['vmax'], f['item_norm'], f['out_idx'], f['out_perm'], f['flags'], f['open_list'],
                              f['open_count'])


def rejected(entry, base, says, **change):
    from polara_amd import _lib
    lib = _lib.load()
    a = dict(base, **change)
    blk = a['settle']                              # (kept alive over the call)
    if blk is not None:
        a['settle'] = ctypes.byref(blk)
    args = [a[name] for name in ORDER[entry]]
    assert len(args) == len(_lib.PROTOTYPES[entry][1]) == (27 if entry == SINGLE else 29)
    rc = getattr(lib, entry)(*args)
    msg = (lib.pk_last_error() or b'').decode()
    assert rc != 0, (entry, change)
    assert msg.startswith(entry + ': ') and says in msg, (entry, change, msg)


# rules of the arguments both entries share: (what the message says, the form of the users' side, the change that breaks the rule)
SHARED = [
    ('exactly one', PACKED, dict(Ep=None, user_bound=None, tile_bound=None)),
    ('exactly one', PACKED, dict(E=P[12], lde=52)),
    ('exactly one', ROWS, dict(Ep=P[10])),
    ('go together', PACKED, dict(user_bound=None)),
    ('go together', PACKED, dict(tile_bound=None)),
    ('go with E_dev', PACKED, dict(extra=P[13], extra_ld=52)),
    ('go with E_dev', PACKED, dict(user_bound_out=P[14])),
    ('user_bound goes with Ep_dev', ROWS, dict(user_bound=P[11])),
    ('16-byte aligned', ROWS, dict(E=P[12] + 8)),
    ('even leading dimension', ROWS, dict(lde=51)),
    ('even leading dimension', ROWS, dict(lde=48)),
    ('stride of the extra term', ROWS, dict(extra_ld=0)),
    ('bad sizes', PACKED, dict(n_users=0)),
    ('bad sizes', ROWS, dict(n_items=0)),
    ('bad sizes', ROWS, dict(n_items=0x7fffff00)),
    ('dense seen masks', ROWS, dict(dense_tiles=-1)),
    ('dense seen masks', ROWS, dict(dense_tiles=8, seen_dense=P[20])),
    ('dense seen masks', PACKED, dict(dense_tiles=8, seen_dense=P[20], seen_skip=P[21], seen_ptr=None, seen_tiles=None, seen_ntiles=None)),
    ('K=999 unsupported', PACKED, dict(K=999)),
    ('K=257 unsupported', ROWS, dict(K=257, lde=258)),
    ('alignment', ROWS, dict(Vp=P[0] + 4)),
    ('alignment', PACKED, dict(Ep=P[10] + 8)),
    ('state buffer', ROWS, dict(state=None)),
    ('state buffer', PACKED, dict(state=P[8] + 8)),
    ('go together (all or none)', ROWS, dict(seen_tiles=None)),
    ('go together (all or none)', PACKED, dict(seen_ntiles=None)),
    ('go together (all or none)', ROWS, dict(seen_ptr=None)),
]


@pytest.mark.parametrize('entry', [SINGLE, TWO])
def test_shared_argument_rules_are_rejected_before_any_launch(entry):
    for says, base, change in SHARED:
        rejected(entry, base, says, **change)


def test_single_sweep_rules():
    for base in (PACKED, ROWS):
        rejected(SINGLE, base, 'splits*KC <= 64', splits=0)
        rejected(SINGLE, base, 'splits*KC <= 64', splits=2)                   # 2 * 48
        rejected(SINGLE, base, 'splits*KC <= 64', KC=32, splits=3)
        rejected(SINGLE, base, 'KC=48 unsupported')                            # the launcher's own refusal: nothing was launched
    # the settle block: the rows side only, ...
    rejected(SINGLE, PACKED, 'go with E_dev', settle=settle_block())
    # ... a single list of 16 or 32 candidates, ...
    rejected(SINGLE, ROWS, 'settle needs splits = 1 and KC = 16 or 32', settle=settle_block(), KC=16, splits=2)
    rejected(SINGLE, ROWS, 'settle needs splits = 1 and KC = 16 or 32', settle=settle_block(), KC=64)
    rejected(SINGLE, ROWS, 'settle needs splits = 1 and KC = 16 or 32', settle=settle_block())
    # ... user ids that fit the open list, the pruning bound and the error weights, ...
    rejected(SINGLE, ROWS, 'int32 open list', settle=settle_block(), KC=16, n_users=2 ** 31)
    rejected(SINGLE, ROWS, 'pruning bound and the fold-in', settle=settle_block(), KC=16, tile_bound=None)
    rejected(SINGLE, ROWS, 'pruning bound and the fold-in', settle=settle_block(), KC=32, extra=None, extra_ld=0)
    # ... 1 <= topk <= KC, vmax >= 0 and the four outputs
    rejected(SINGLE, ROWS, '1 <= topk <= KC', settle=settle_block(topk=0), KC=16)
    rejected(SINGLE, ROWS, '1 <= topk <= KC', settle=settle_block(topk=17), KC=16)
    rejected(SINGLE, ROWS, '1 <= topk <= KC', settle=settle_block(topk=33), KC=32)
    rejected(SINGLE, ROWS, 'vmax >= 0', settle=settle_block(vmax=-1e-300), KC=16)
    for out in ('out_idx', 'flags', 'open_list', 'open_count'):
        rejected(SINGLE, ROWS, 'settle: null outputs', settle=settle_block(**{out: None}), KC=16)


def test_two_phase_rules():
    # the pruning bounds are required on either side
    rejected(TWO, PACKED, 'needs the pruning bounds', user_bound=None, tile_bound=None)
    rejected(TWO, ROWS, 'needs the pruning bounds', tile_bound=None)
    for base in (PACKED, ROWS):
        rejected(TWO, base, '(splits + 1) * KC <= 256', splits=0)
        rejected(TWO, base, '(splits + 1) * KC <= 256', splits=5)             # 6 * 48
        rejected(TWO, base, '(splits + 1) * KC <= 256', KC=16, splits=16)
        rejected(TWO, base, '(splits + 1) * KC <= 256', KC=65)
        rejected(TWO, base, '1 <= head_tiles < n_tiles', head_tiles=0)
        rejected(TWO, base, '1 <= head_tiles < n_tiles', head_tiles=41)       # 1289 items: 41 tiles
        for buf in ('work_score', 'work_idx', 'cand_score', 'cand_idx'):
            rejected(TWO, base, 'null list buffers', **{buf: None})
    # it has no settle argument: two arguments more than the single sweep (head_tiles, the work lists), one less (settle)
    assert 'settle' not in ORDER[TWO] and len(ORDER[TWO]) == len(ORDER[SINGLE]) + 3 - 1
