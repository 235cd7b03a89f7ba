"""Write dynibar_amd/view_log_tables.py: the 256 x 3 float64 lookup tables of matplotlib's `jet` and `gray` colour maps, exactly
``matplotlib.colormaps[name](np.arange(256))[:, :3]``, as hexadecimal float literals (every bit kept).  The product does not import
matplotlib: run this where matplotlib is installed when a table has to be made again.     python tools/make_view_log_tables.py"""
import os

import matplotlib
import numpy as np

NAMES = ('jet', 'gray')
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dynibar_amd', 'view_log_tables.py')


def table(name):
  t = np.asarray(matplotlib.colormaps[name](np.arange(256))[:, :3], dtype=np.float64)
  assert t.shape == (256, 3)
  return t


def main():
  lines = ['"""The lookup tables of the colour maps `colorize` knows (utils.py:124-125 takes them from matplotlib): 256 rows of (r, g, b) as float64,',
           f'written by tools/make_view_log_tables.py from matplotlib {matplotlib.__version__}.  Generated: do not edit."""',
           '', 'TABLES = {']
  for name in NAMES:
    lines.append(f"    '{name}': (")
    for row in table(name):
      lines.append('        ' + ' '.join(f"'{float(v).hex()}'," for v in row))
    lines.append('    ),')
  lines += ['}', '']
  with open(OUT, 'w') as f:
    f.write('\n'.join(lines))
  print(OUT)


if __name__ == '__main__':
  main()
