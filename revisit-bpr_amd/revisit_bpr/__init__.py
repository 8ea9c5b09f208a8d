"""MI355X-native BPR-MF engine behind the import paths of Nemexur/revisit-bpr's ``revisit_bpr``."""


def __getattr__(name):  # resolved on first use: importing the package loads neither torch nor the library
    if name == "fold_in":
        from revisit_bpr.foldin import fold_in

        return fold_in
    if name == "fold_in_items":
        from revisit_bpr.foldin_items import fold_in_items

        return fold_in_items
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
