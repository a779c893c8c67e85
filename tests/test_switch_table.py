"""INTEGRATION.md's table of environment switches lists exactly the VKX_* variables the library and bench.py read (a source scan; no
GPU, nothing is loaded)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a read of the environment with the variable's name next to it: getenv("VKX_X") and the two helpers of csrc/vkx_internal.h in the
# C++ sources, os.environ.get('VKX_X' ...), os.environ['VKX_X'] (not an assignment) and 'VKX_X' in os.environ in the Python ones
CXX_READ = re.compile(r'\b(?:getenv|vkx_env_int|vkx_env_on)\s*\(\s*"(VKX_[A-Z0-9_]+)"')
PY_READS = (re.compile(r'''os\.environ\.get\(\s*['"](VKX_[A-Z0-9_]+)['"]'''),
            re.compile(r'''os\.environ\[\s*['"](VKX_[A-Z0-9_]+)['"]\s*\](?!\s*=[^=])'''),
            re.compile(r'''['"](VKX_[A-Z0-9_]+)['"]\s+in\s+os\.environ'''))


def switches_read():
    names = set()
    paths = [os.path.join(ROOT, 'bench.py')]
    for dirpath, _dirs, files in os.walk(os.path.join(ROOT, 'vkit_amd')):
        paths += [os.path.join(dirpath, f) for f in files if f.endswith(('.py', '.hip', '.h', '.cpp'))]
    for path in paths:
        text = open(path, errors='replace').read()
        if path.endswith('.py'):
            for pattern in PY_READS:
                names.update(pattern.findall(text))
        else:
            names.update(CXX_READ.findall(text))
    return names


def switches_documented():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = text.split('## Environment switches', 1)[1].split('\n## ', 1)[0]
    names = set()
    for line in section.splitlines():
        if line.startswith('| `'):
            first_column = re.split(r'(?<!\\)\|', line)[1]
            names.update(re.findall(r'\bVKX_[A-Z0-9_]+', first_column))
    return names


def test_every_switch_read_has_a_row_and_every_row_a_read():
    read, documented = switches_read(), switches_documented()
    assert len(read) > 20 and len(documented) > 20      # the scan found the sources and the table
    assert read - documented == set(), 'read from the environment without a row in INTEGRATION.md'
    assert documented - read == set(), 'a row in INTEGRATION.md that nothing reads'
