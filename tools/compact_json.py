"""JSON for profiles/: one line per top-level key, one per element of a list of records (a diff shows which record moved)."""
import json

def dump(doc):
    """The document with one line per top-level key and one per element of a top-level list or of a list one level below."""
    one = lambda v: json.dumps(v, separators=(", ", ": "))
    def value(v, pad):
        if isinstance(v, list) and v and isinstance(v[0], dict):
            return "[\n" + ",\n".join(pad + " " + one(e) for e in v) + "\n" + pad + "]"
        if isinstance(v, dict) and any(isinstance(e, list) and e and isinstance(e[0], dict) for e in v.values()):
            return "{\n" + ",\n".join(pad + " " + json.dumps(k) + ": " + value(e, pad + " ") for k, e in v.items()) + "\n" + pad + "}"
        return one(v)
    return "{\n" + ",\n".join(" " + json.dumps(k) + ": " + value(v, " ") for k, v in doc.items()) + "\n}\n"
