#!/usr/bin/env python3
"""gpurun_out/pmc_raw.json (tools/pmc_extract.py) -> profiles/pmc_traffic.json: HBM bytes per launch of each
disco kernel, corrected as /opt/skills/guides/MI355X_MICROARCH.md (HBM section) prescribes:
  * FETCH_SIZE and WRITE_SIZE come from SEPARATE rocprofv3 --pmc passes (TCC slots) and are in KiB;
  * on gfx950 FETCH_SIZE reports exactly half of the bytes of a coalesced streaming read -> x2;
  * WRITE_SIZE is taken x1.
Both corrections were re-calibrated in the same runs on kernels whose traffic is known exactly:
  torch abs() over a 1.28 GB tensor (FETCH x2 = bytes read, WRITE x1 = bytes written), and this repo's k_istft
  (reads every spectrum once plus the 8/7 frame overlap; writes exactly R*K*L*4 bytes).
Usage: tools/pmc_traffic.py gpurun_out/pmc_raw.json profiles/pmc_traffic.json"""
import json
import re
import sys

import hashlib
import os

# kernel-name prefix -> the library's stage name (disco_stage_report / bench.py `stages`); several kernels can serve one stage
STAGE_OF = {'k_stft_cov<': 'stft_cov1', 'k_stft<': 'stft', 'k_mask_oracle<': 'mask_oracle', 'k_istft<': 'istft',
            'k_step2_cov_fused<': 'step2_cov', 'k_step2_apply_istft<': 'step2_apply_istft', 'k_step2_apply_fused<': 'step2_apply',
            'k_stft_apply_istft<': 'stft_apply_istft', 'k_cov_split<': 'cov_split', 'k_cov_split_lds<': 'cov_split', 'k_stft_pairs<': 'stft', 'k_cov_big<': 'cov_big', 'k_cov<': 'cov',
            'k_room_cov_dma<': 'room_cov2', 'k_room_cov<': 'room_cov2', 'k_apply_mq<': 'apply2', 'k_apply_m<': 'apply2', 'k_apply<': 'apply', 'k_gevd_mwf_r1_dpp<': 'solve2', 'k_gevd_mwf_r1_thread<': 'solve_thread', 'k_gevd_mwf_r1<': 'solve'}


def csrc_digest():
    """Same digest as bench.py: identifies the kernel sources the counters were measured on."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = hashlib.sha256()
    d = os.path.join(repo, 'disco_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()[:16]


raw = json.load(open(sys.argv[1]))
out = {'_method': 'rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (two passes) on '
                  '`bench.py --steps 1 --warmup 0 --no-stage-timing`; bytes = (2*FETCH_SIZE + WRITE_SIZE) * 1024',
       '_calibration': {}, '_csrc_digest': csrc_digest()}
for k, v in raw.items():
    if k.startswith('_'):
        continue
    if 'AbsFunctor' in k:
        out['_calibration']['torch_abs_1.28GB'] = {c: x['per_dispatch'] * 1024 for c, x in v.items()}
    if 'neg' in k.lower() and 'disco::' not in k and max(x['per_dispatch'] for x in v.values()) * 1024 > 1e9:
        # bench.py --pmc-calibrate: torch.neg over 2^30 floats = 4 GiB read + 4 GiB written by one kernel, known exactly
        out['_calibration']['torch_neg_4GiB'] = dict({c: x['per_dispatch'] * 1024 for c, x in v.items()}, known_bytes_each_way_per_dispatch=2 * 2 ** 30,
                                                      note='torch splits the 4 GiB tensor into two dispatches of 2 GiB (32-bit indexing): FETCH_SIZE x2 and WRITE_SIZE x1 reproduce 2 GiB each way',
                                                      kernel=k[:80])
    if 'k_selftest_stream<' in k:
        # bench.py --pmc-calibrate: 2^30 floats moved ONE dword per lane and load (the access width of the STFT kernels' sample reads)
        wr = 'k_selftest_stream<true>' in k
        out['_calibration']['dword_per_lane_copy_4GiB' if wr else 'dword_per_lane_read_4GiB'] = dict(
            {c: x['per_dispatch'] * 1024 for c, x in v.items()}, known_bytes_read_per_dispatch=4 * 2 ** 30,
            known_bytes_written_per_dispatch=4 * 2 ** 30 if wr else 0, kernel=k[:80])
        continue
    if 'disco::' not in k:
        continue
    name = k.replace('void disco::', '')
    f = v.get('FETCH_SIZE', {}).get('per_dispatch')
    w = v.get('WRITE_SIZE', {}).get('per_dispatch')
    ent = {'kernel': name, 'fetch_size_KiB_raw': f, 'write_size_KiB_raw': w,
           'hbm_read_bytes_per_launch': None if f is None else 2 * f * 1024,
           'hbm_write_bytes_per_launch': None if w is None else w * 1024}
    if f is not None and w is not None:
        ent['hbm_bytes_per_launch'] = 2 * f * 1024 + w * 1024
    stage = next((s for p, s in STAGE_OF.items() if name.startswith(p)), name)
    # bench.py looks the dominant stage up by ITS name: map kernels to the stage they serve in the profiled configuration
    if stage == 'stft_cov1' and re.match(r'k_stft_cov<\d+, \d+, false', name):     # STORE = false (the 3rd argument; a 4th, the layout, may follow)
        stage = 'stft_cov1_nostore'
    if stage in ('solve', 'solve_thread'):
        stage = 'solve1' if (stage == 'solve_thread' or '<4,' in name or '<8,' in name) else 'solve2'
    if stage == 'cov_split':
        stage = 'cov1' if re.search(r'<\d+, 0,', name) else 'cov2'
    if stage in out and 'hbm_bytes_per_launch' in out[stage] and 'hbm_bytes_per_launch' in ent:
        continue          # first (largest-share) kernel of a stage wins
    out[stage] = ent
json.dump(out, open(sys.argv[2], 'w'), indent=1)
print(json.dumps({k: (round(v['hbm_bytes_per_launch'] / 1e9, 2) if isinstance(v, dict) and 'hbm_bytes_per_launch' in v else None)
                  for k, v in out.items() if not k.startswith('_')}))
