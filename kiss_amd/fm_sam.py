"""The header lines of the SAM output, as `kiss fmindex_query ... --sam` writes them in front of the alignment lines (print_sam in
kiss_amd/csrc/host/cli_format.hpp): for a caller who turns the records of FMIndex.map / map_pairs into a file.  Plain Python; no
library call."""


def _bytes(x):
    return bytes(x) if isinstance(x, (bytes, bytearray)) else str(x).encode()


def sam_header(ref_names, bounds, version):
    """@HD, one @SQ per record -- its name and its length bounds[r + 1] - bounds[r] -- and @PG, as bytes.  ref_names: the R names
    (str or bytes), or None for a text without records; bounds: the R + 1 starts of the records, as map(bounds=...) takes them"""
    names = [_bytes(x) for x in (ref_names or [])]
    if names and len(bounds) != len(names) + 1:
        raise ValueError("bounds has R + 1 = %d entries" % (len(names) + 1))
    out = [b"@HD\tVN:1.6\tSO:unsorted\n"]
    for r, name in enumerate(names):
        out.append(b"@SQ\tSN:" + name + b"\tLN:" + str(int(bounds[r + 1]) - int(bounds[r])).encode() + b"\n")
    out.append(b"@PG\tID:kiss\tPN:kiss\tVN:" + _bytes(version) + b"\n")
    return b"".join(out)
