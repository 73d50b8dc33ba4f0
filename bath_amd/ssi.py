"""Easel's SSI v3 indexes ("sequence/subsequence index"), as bathfetch --index writes them and bathfetch reads them: host code.

The layout, every field big-endian (the recorded tutorial/tRNA-proteins.bhmm.ssi, 917 bytes for 12 names and 12 accessions, is the
specification; tests/golden holds it):

    header             magic 0xd3d3c9b3 u32, flags u32, offsz u32, nfiles u16, nprimary u64, nsecondary u64,
                       flen plen slen frecsize precsize srecsize u32 each, foffset poffset soffset offsz bytes each
    file records       name padded with NULs to flen, then format, flags, bpl, rpl u32 each
    primary records    sorted by key in strcmp order: key padded to plen, file number u16, record offset, data offset (offsz bytes each),
                       length u64
    secondary records  sorted: key padded to slen, primary key padded to plen

flen, plen and slen are the longest string plus its NUL.  The writer covers one file with 64-bit offsets (what the recorded file
has; data offset and length 0, as a model file's are); the reader takes 64-bit offsets too (no recorded file shows the 32-bit
layout) and any number of files, and finds a key by binary search among the primary keys, then among the secondary ones.
"""
import struct

MAGIC = 0xd3d3c9b3
_HEAD = struct.Struct(">IIIHQQ6I")            # up to srecsize: 54 bytes; the three section offsets follow
_FILE_TAIL = struct.Struct(">4I")


class SSIFormatError(Exception):
    pass


def _pad(key, n):
    return key + b"\0" * (n - len(key))


def build(file_name, primary, secondary=()):
    """The bytes of an index of one file.  primary: (key, record offset) pairs; secondary: (alias, primary key) pairs; keys are str
    (latin-1) or bytes.  Raises ValueError on a repeated key, as esl_newssi_Write refuses one."""
    enc = lambda s: s if isinstance(s, bytes) else s.encode("latin-1")
    name = enc(file_name)
    pri = sorted((enc(k), int(off)) for k, off in primary)
    sec = sorted((enc(a), enc(k)) for a, k in secondary)
    for what, keys in (("primary", [k for k, _ in pri]), ("secondary", [a for a, _ in sec])):
        for a, b in zip(keys, keys[1:]):
            if a == b:
                raise ValueError("%s key %s occurs more than once" % (what, a.decode("latin-1")))
    offsz = 8
    flen = len(name) + 1
    plen = max([len(k) for k, _ in pri] or [0]) + 1
    slen = max([len(a) for a, _ in sec] or [0]) + 1
    frecsize, precsize, srecsize = flen + 16, plen + 2 + 2 * offsz + 8, slen + plen
    foffset = _HEAD.size + 3 * offsz
    poffset = foffset + frecsize
    soffset = poffset + precsize * len(pri)
    out = [_HEAD.pack(MAGIC, 0, offsz, 1, len(pri), len(sec), flen, plen, slen, frecsize, precsize, srecsize),
           struct.pack(">3Q", foffset, poffset, soffset),
           _pad(name, flen), _FILE_TAIL.pack(0, 0, 0, 0)]
    for k, off in pri:
        out.append(_pad(k, plen) + struct.pack(">HQQQ", 0, off, 0, 0))
    for a, k in sec:
        out.append(_pad(a, slen) + _pad(k, plen))
    return b"".join(out)


class Index:
    """An index read from <path>.  find(key) -> (file name, record offset) or None."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as fh:
            d = fh.read()
        bad = lambda why: SSIFormatError("%s is not an SSI index this reader takes: %s" % (path, why))
        if len(d) < _HEAD.size:
            raise bad("the file ends inside the header")
        (magic, self.flags, offsz, nfiles, self.nprimary, self.nsecondary,
         self.flen, self.plen, self.slen, frec, prec, srec) = _HEAD.unpack_from(d)
        if magic != MAGIC:
            raise bad("wrong magic number")
        if offsz != 8:
            raise bad("offsets of %d bytes, not 8" % offsz)
        o = ">Q"
        if len(d) < _HEAD.size + 3 * offsz:
            raise bad("the file ends inside the header")
        foff, poff, soff = (struct.unpack_from(o, d, _HEAD.size + i * offsz)[0] for i in range(3))
        if frec != self.flen + 16 or prec != self.plen + 2 + 2 * offsz + 8 or srec != self.slen + self.plen or min(self.flen, self.plen) < 1:
            raise bad("record sizes that do not follow from the key lengths")
        for start, size, n, what in ((foff, frec, nfiles, "file"), (poff, prec, self.nprimary, "primary"), (soff, srec, self.nsecondary, "secondary")):
            if n and (start < _HEAD.size + 3 * offsz or start + size * n > len(d)):
                raise bad("the file ends inside the %s records (truncated?)" % what)
        self._d, self._o, self._offsz = d, o, offsz
        self._poff, self._prec, self._soff, self._srec = poff, prec, soff, srec
        self.files = [d[foff + i * frec: foff + i * frec + self.flen].split(b"\0", 1)[0].decode("latin-1") for i in range(nfiles)]

    def _search(self, key, start, size, klen, n):
        lo, hi = 0, n
        while lo < hi:
            mid = (lo + hi) // 2
            at = start + mid * size
            k = self._d[at: at + klen].split(b"\0", 1)[0]
            if k == key:
                return at
            if k < key:
                lo = mid + 1
            else:
                hi = mid
        return None

    def find(self, key):
        key = key if isinstance(key, bytes) else key.encode("latin-1")
        at = self._search(key, self._poff, self._prec, self.plen, self.nprimary)
        if at is None:
            s = self._search(key, self._soff, self._srec, self.slen, self.nsecondary)
            if s is None:
                return None
            pkey = self._d[s + self.slen: s + self._srec].split(b"\0", 1)[0]
            at = self._search(pkey, self._poff, self._prec, self.plen, self.nprimary)
            if at is None:
                raise SSIFormatError("%s: secondary key %s names a primary key the index does not hold" % (self.path, key.decode("latin-1")))
        fnum, = struct.unpack_from(">H", self._d, at + self.plen)
        off, = struct.unpack_from(self._o, self._d, at + self.plen + 2)
        if fnum >= len(self.files):
            raise SSIFormatError("%s: key %s names file %d of %d" % (self.path, key.decode("latin-1"), fnum, len(self.files)))
        return self.files[fnum], off

    def primary_keys(self):
        return [self._d[self._poff + i * self._prec: self._poff + i * self._prec + self.plen].split(b"\0", 1)[0].decode("latin-1")
                for i in range(self.nprimary)]
