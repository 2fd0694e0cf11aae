"""Runner of the dense-operator legs whose switch is read once per process (tests/_dense_cases.py LEGS): started by
tests/test_dense_gpu.py as a fresh child process with the leg's variables in its environment,

    python tests/_dense_child.py LEG [--fake] [--cu N]

runs the leg's cases over librlhip.so (--fake: over tests/fake_lib.py, which is how the CPU tier checks this runner),
prints the largest error / bound per kernel family and DENSE_CHILD_OK, or exits with status 1 and the failing case's
message."""
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def main(argv):
    import _dense_cases as cases
    leg = argv[0]
    if leg not in cases.LEGS:
        print('unknown leg %r' % leg)
        return 2
    want, run = cases.LEGS[leg]
    for name, value in want.items():
        if os.environ.get(name) != value:
            print('leg %s needs %s=%s in the environment' % (leg, name, value))
            return 2
    if '--fake' in argv:
        import fake_lib
        fake_lib.install()
    cu = int(argv[argv.index('--cu') + 1]) if '--cu' in argv else compute_units()
    try:
        run(cu)
    except Exception as e:
        traceback.print_exc()
        print('DENSE_CHILD_FAILED leg %s: %s' % (leg, e))
        return 1
    print(cases.ratios_text())
    print('DENSE_CHILD_OK leg %s' % leg)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
