"""kiss_amd -- MI355X-native k-ordered suffix sorting (hot path of jhhung/kISS).

Only what the path needs: csrc/ (HIP kernels + the C ABI, built into libkiss_hip.so) and the
host-side mirror of the reference's sorter facade.
"""
from ._lib import ALGO_PARALLEL_SORTING, ALGO_PREFIX_DOUBLING, KissHipError, LIB_PATH, load  # noqa: F401
from .sorter import (K_UNBOUNDED, Context, KISS1Sorter, KISS2Sorter, MultiContext, lcp_array, lcp_array_bytes,  # noqa: F401
                     suffix_array_bytes)
from .fm_index_bytes import FMIndexBytes  # noqa: F401,E402
from .fm_chain import chain_seeds  # noqa: F401,E402
from .fm_align import ALIGN_DEFAULTS, align_chains, align_params  # noqa: F401,E402
from .fm_select import SELECT_DEFAULTS, select_alignments, select_params  # noqa: F401,E402
from .fm_pair import PAIR_DEFAULTS, pair_hits, pair_params  # noqa: F401,E402
from .fm_rescue import RESCUE_DEFAULTS, merge_alignments, plan_rescue, rescue_params  # noqa: F401,E402
from .reads import interleave_reads, interleave_reads_dev, parse_reads, parse_reads_dev  # noqa: F401,E402
from .fm_md import md_strings, md_tags  # noqa: F401,E402
from .fm_insert import INSERT_DEFAULTS, estimate_insert, insert_params  # noqa: F401,E402
from .fm_sam import sam_header  # noqa: F401,E402
from . import sam_writer  # noqa: F401,E402  (the SAM lines on the device: kiss_amd.sam_writer.sam_lines, sam_lines_dev)
from . import batches  # noqa: F401,E402  (read files in batches: kiss_amd.batches.read_batches, map_file)
