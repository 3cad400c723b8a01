"""Test helpers for BAM input (never used by the product): a BAM writer that follows SAMv1 by hand (BGZF members with the BC extra
field and the EOF block, header text, reference entries, records with CIGAR and aux tags), a decoder that gives what
`samtools fastq` gives by default (secondary / supplementary records dropped, reverse-strand records restored to the sequencer's
orientation), written independently of the native reader, and an emulated engine that takes nib4 uploads."""
import gzip
import random
import struct
import uuid
import zlib

from emu_engine import EmuEngine
from topsicle_amd import seqio

NT16 = "=ACMGRSVTWYHKDBN"
CODE = {c: i for i, c in enumerate(NT16)}
COMP = str.maketrans("=ACMGRSVTWYHKDBN", "=TGKCYSBAWRDMHVN")      # IUPAC complement, letter by letter
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FLAG_REVERSE, FLAG_UNMAPPED, FLAG_SECONDARY, FLAG_SUPPLEMENTARY = 0x10, 0x4, 0x100, 0x800


def bgzf_block(data: bytes) -> bytes:
    """One BGZF member: a gzip member with the BC extra field giving its total size - 1."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    cdata = co.compress(data) + co.flush()
    bsize = 12 + 6 + len(cdata) + 8
    head = b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def bgzf(data: bytes, block: int = 65280, cuts=None) -> bytes:
    """The stream in BGZF blocks of `block` bytes of text (or at the offsets `cuts`), then the EOF block."""
    edges = sorted(set([0, len(data)] + [c for c in (cuts or range(block, len(data), block)) if 0 < c < len(data)]))
    out = [bgzf_block(data[a:b]) for a, b in zip(edges, edges[1:])]
    return b"".join(out) + BGZF_EOF


def header_bytes(refs=(("chr1", 30_000_000), ("chr2", 20_000_000)), text=None) -> bytes:
    if text is None:
        text = ("@HD\tVN:1.6\tSO:unknown\n@PG\tID:basecaller\tPN:dorado\tVN:0.7.0\tCL:dorado basecaller sup pod5/\n"
                "@RG\tID:run1_model\tPU:FAX00000\tPL:ONT\tDS:basecall_model=sup\n")
    t = text.encode()
    out = [b"BAM\x01", struct.pack("<i", len(t)), t, struct.pack("<i", len(refs))]
    for name, ln in refs:
        n = name.encode() + b"\x00"
        out += [struct.pack("<i", len(n)), n, struct.pack("<i", ln)]
    return b"".join(out)


def _aux(tags) -> bytes:
    out = []
    for tag, typ, val in tags:
        out.append(tag.encode() + typ.encode())
        if typ == "Z":
            out.append(val.encode() + b"\x00")
        elif typ == "i":
            out.append(struct.pack("<i", val))
        elif typ == "f":
            out.append(struct.pack("<f", val))
        elif typ == "B":
            sub, arr = val                                            # (uint8 arrays: ML)
            out.append(sub.encode() + struct.pack("<i", len(arr)) + bytes(arr))
    return b"".join(out)


def record_bytes(name: str, flag: int, seq: str, qual, ref_id=-1, pos=-1, cigar=(), tags=()) -> bytes:
    """One BAM record.  `seq` / `qual` as STORED (for a reverse-strand record: the reverse complement of the read); qual = None
    stores 0xFF (no qualities)."""
    L = len(seq)
    codes = [CODE[c] for c in seq] + ([0] if L & 1 else [])
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    q = b"\xff" * L if qual is None else bytes(ord(c) - 33 for c in qual)
    nm = name.encode() + b"\x00"
    cig = b"".join(struct.pack("<I", (n << 4) | "MIDNSHP=X".index(op)) for n, op in cigar)
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), 60 if ref_id >= 0 else 255, 4680, len(cigar), flag, L, -1, -1, 0)
    body += nm + cig + packed + q + _aux(tags)
    return struct.pack("<i", len(body)) + body


def revcomp(s: str) -> str:
    return s.translate(COMP)[::-1]


def dorado_tags(rng, L):
    return [("qs", "f", 12.5), ("mx", "i", 1), ("ch", "i", rng.randint(1, 512)), ("st", "Z", "2024-01-01T00:00:00Z"),
            ("RG", "Z", "run1_model"), ("MM", "Z", "C+m?;"), ("ML", "B", ("C", [rng.randint(0, 255) for _ in range(min(L, 7))]))]


def make_reads(seed=1, n=60, lengths=None, iupac=True, aligned=True):
    """Records of a test BAM: [(name, flag, read (sequencer's orientation), qual or None, cigar, tags)].  Covers forward, reverse,
    secondary, supplementary and unmapped records, l_seq = 0, odd lengths, IUPAC and '=' bases, missing qualities, records longer
    than one BGZF block."""
    rng = random.Random(seed)
    lengths = lengths or [0, 1, 2, 15, 16, 17, 31, 63, 64, 65, 127, 128, 129, 999, 1001, 70_001, 3, 70_000]
    out = []
    motif = "CCCTAAA"
    for i in range(n):
        L = lengths[i % len(lengths)] if i < len(lengths) else rng.randint(0, 5000)
        if rng.random() < 0.3 and L > 50:
            tract = min(L, rng.randint(20, 800))
            s = (motif * (tract // 7 + 1))[:tract] + "".join(rng.choice("ACGT") for _ in range(L - tract))
        else:
            s = "".join(rng.choice("ACGT") for _ in range(L))
        if iupac and L > 4 and i % 3 == 0:
            s = list(s)
            for _ in range(1 + L // 500):
                s[rng.randrange(L)] = rng.choice("NRYKMSWBDHV=")
            s = "".join(s)
        qual = None if (i % 11 == 5 and L) else "".join(chr(33 + rng.randint(0, 60)) for _ in range(L))
        flag = 0
        if aligned:
            flag = rng.choice([0, 0, FLAG_REVERSE, FLAG_REVERSE, FLAG_SECONDARY, FLAG_SUPPLEMENTARY | FLAG_REVERSE, FLAG_UNMAPPED,
                               FLAG_SECONDARY | FLAG_REVERSE])
        else:
            flag = FLAG_UNMAPPED
        name = str(uuid.UUID(int=rng.getrandbits(128)))
        cigar = [(L, "M")] if (aligned and L and not flag & FLAG_UNMAPPED) else []
        out.append((name, flag, s, qual, cigar, dorado_tags(rng, L)))
    return out


def write_bam(path, reads, block=65280, cuts=None, header=None):
    """reads: as make_reads gives them (read in the sequencer's orientation: reverse-strand records are stored reverse-complemented)."""
    body = [header_bytes() if header is None else header]
    for name, flag, s, qual, cigar, tags in reads:
        rev = bool(flag & FLAG_REVERSE)
        stored = revcomp(s) if rev else s
        sq = None if qual is None else (qual[::-1] if rev else qual)
        mapped = bool(cigar)
        body.append(record_bytes(name, flag, stored, sq, ref_id=0 if mapped else -1, pos=100 if mapped else -1, cigar=cigar, tags=tags))
    data = b"".join(body)
    with open(path, "wb") as fh:
        fh.write(bgzf(data, block, cuts))
    return data


def decode_bam(path):
    """What `samtools fastq` writes by default for a BAM file, as [(name, seq, qual)]: the BGZF members inflated by gzip, records
    parsed field by field, secondary / supplementary dropped, reverse-strand ones reverse-complemented (qualities reversed), a
    record without qualities given '!' for every base (the project's convention)."""
    data = gzip.decompress(open(path, "rb").read())
    assert data[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", data, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", data, p)[0]
        p += 4 + ln + 4
    out = []
    while p < len(data):
        bs = struct.unpack_from("<i", data, p)[0]
        ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", data, p + 4)
        name = data[p + 36:p + 36 + l_name - 1].decode()
        s0 = p + 36 + l_name + 4 * n_cig
        seq = "".join(NT16[(data[s0 + j // 2] >> (4 * (1 - j % 2))) & 15] for j in range(l_seq))
        qb = data[s0 + (l_seq + 1) // 2:s0 + (l_seq + 1) // 2 + l_seq]
        qual = "!" * l_seq if (l_seq and qb[0] == 0xFF) else "".join(chr(b + 33) for b in qb)
        p += 4 + bs
        if flag & (FLAG_SECONDARY | FLAG_SUPPLEMENTARY):
            continue
        if flag & FLAG_REVERSE:
            seq, qual = revcomp(seq), qual[::-1]
        out.append((name, seq, qual))
    return out


def write_fastq(path, recs):
    with open(path, "w") as fh:
        for name, seq, qual in recs:
            fh.write(f"@{name}\n{seq}\n+\n{qual}\n")


class NibEmuEngine(EmuEngine):
    """EmuEngine that also takes nib4 uploads: the host packer (tps_pack_nib4) expands the codes, then the packed upload."""

    def upload_nib4(self, slot, nib, src, desc, n_words):
        seq2, inv, d = seqio.pack_nib4_host(nib, src, desc, n_words)
        self.upload_packed(slot, seq2, inv if (d["flags"] & 1).any() else None, d)

    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(NibEmuEngine())
        return hs[j]


def fastq_records_to_bam(fastq_path, bam_path, block=65280):
    """The records of a FASTQ(.gz) file as an unaligned BAM (uBAM, flag 4), named by their ids."""
    reads = [(r.id, FLAG_UNMAPPED, r.seq, r.qual, [], [("RG", "Z", "run1_model")]) for r in seqio.read_records(fastq_path)]
    write_bam(bam_path, reads, block=block)
    return reads
