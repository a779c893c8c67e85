"""Reader of tests/golden/page_cropping.npz (written by tests/golden/make_cropping_golden.py from the reference's own
PageCroppingStep.run): one dict per case.  The file holds a JSON index and a few flat arrays; every plane is an
(array, offset, shape) reference into them."""
import json
import os

import numpy as np

from crop_restate import LABELS

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'page_cropping.npz')


def cases():
    data = np.load(PATH)
    flat = {key: data[key] for key in data.files if key != 'index'}

    def plane(ref):
        key, offset, shape = ref
        size = int(np.prod(shape, dtype=np.int64))
        return flat[key][offset:offset + size].reshape(shape)

    out = []
    for row in json.loads(str(data['index'])):
        case = dict(name=row['case'], seed=int(row['seed']), is_prob=bool(row['is_prob']), overrides=row['config'],
                    planes={n: plane(ref) for n, ref in row['inputs'].items()},
                    attempts=np.asarray(row['attempts'], np.int64).reshape(-1, 12), rng_state=row['rng_state'], samples=[])
        for s in row['samples']:
            sample = {n: plane(ref) for n, ref in s['planes'].items()}
            sample['target_core_box'] = np.asarray(s['target_core_box'])
            if 'down_shape' in s:
                sample['down_shape'] = tuple(s['down_shape'])
                sample['down_target_core_box'] = np.asarray(s['down_target_core_box'])
            case['samples'].append(sample)
        out.append(case)
    return out


def box4(b):
    return [int(b.up), int(b.down), int(b.left), int(b.right)]


def is_prob_of(case):
    return {n: case['is_prob'] and n == 'page_char_height_score_map' for n in LABELS}
